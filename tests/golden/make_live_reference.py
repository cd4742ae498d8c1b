#!/usr/bin/env python
"""Record what the cross-checks against the REAL reference compare with, so that the suite needs no reference checkout.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_live_reference.py --ref <reference checkout>

Writes, under tests/golden/live/:
  aten_<case>.npz     the reference module's output on the seeded input (tests/test_aten_seq_cpu.py CASES: weights seed 1234, input
                      seed 4321) and fp64 checksums of its parameters (state_dict order) and of the input: the test rebuilds both from
                      the seeds with the drop-in module, which draws the same init stream, and checks them against the checksums;
  fourier.npz         the reference's pre-projection Fourier position features, whole (tests/test_helper_modules.py);
  chan.npz            input, weights and SE / CBAM / ECA outputs of the ragged channel-attention shapes (tests/test_oracle_golden.py);
  lepe.npz            qkv, get_v weights and LePEAttention output of the three LePE modes (tests/test_oracle_golden.py);
  routes.npz          per row of tests/route_cases.py (non-trivial parameters, prep_nontrivial): 257 strided samples, sum and
                      absolute sum of the reference module's output, and fp64 checksums of its parameters and of the input
                      (tests/test_routes_cpu.py); --routes-only rewrites this file alone;
  models.npz          per row of tests/model_cases.py (whole models, prep_nontrivial + prep_model): the reference's output (whole when
                      it holds at most 257 values, else 257 strided samples), its sum and absolute sum, fp64 checksums of the state_dict
                      and of the input, and for `error` rows the name of the exception the reference raises (tests/test_models_cpu.py);
                      --models-only rewrites this file alone;
  mhsa.npz            per row of tests/mhsa_cases.py (the multi-head copies of modules/mhsa.py, non-trivial parameters): the routes.npz
                      record of the reference's own class (Broad_Attention: of the concatenation cases.flat_out makes), and for the
                      error rows the name of the exception the reference raises ("" where it runs) (tests/test_mhsa_cases_cpu.py);
                      --mhsa-only rewrites this file alone;
and tests/golden/reference_names.json: the public names of every reference module a drop-in shim mirrors (tests/test_signatures.py).
"""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TOPS = ("attention_mechanisms", "vision_transformers", "mlps", "cnns")

REF_CLASSES = {"se": ("attention_mechanisms.se_module", "SELayer", (64,), {}), "eca": ("attention_mechanisms.eca", "ECALayer", (64,), {}),
               "cbam": ("attention_mechanisms.cbam", "CBAM", (64,), {}),
               "da": ("attention_mechanisms.double_attention", "DoubleAttention", (64, 32, 32), {}),
               "vit_attn": ("vision_transformers.ViT", "Attention", (192, 6), {}),
               "vit_enc": ("vision_transformers.ViT", "TransformerEncoder", (192, 6), {}),
               "vit": ("vision_transformers.ViT", "VisionTransformer", (),
                       dict(image_size=32, patch_size=8, depths=2, num_heads=4, embedding_dim=64, num_classes=10)),
               "xca": ("vision_transformers.xcit", "XCA", (96, 4), dict(qkv_bias=True)),
               "xca_block": ("vision_transformers.xcit", "XCABlock", (96, 4), dict(qkv_bias=True, eta=1.0)),
               "mixer": ("mlps.mlp_mixer", "MixerLayer", (64, 49), {})}
FOURIER_GRIDS = ((14, 14, 32, 10000), (5, 11, 8, 50), (1, 1, 4, 10000), (31, 2, 6, 1000))
CHAN_SHAPES = (((1, 48, 7, 9), 48, 16), ((3, 32, 5, 5), 32, 4), ((2, 80, 13, 1), 80, 16))
LEPE_MODES = ((8, 0, 2, 32, 2), (8, 1, 4, 32, 1), (6, -1, 6, 64, 4))      # reso, idx, split, dim, heads


def _model_records(model_cases, ref_cls, sample_index):
    """models.npz: per row of tests/model_cases.py, built from the reference's class by model_cases.build_row."""
    rec = {"ids": np.array([r["id"] for r in model_cases.ROWS])}
    for r in model_cases.ROWS:
        cls = ref_cls(r["mod"], r["cls"])
        if "error" in r:
            try:
                model_cases.build_row(r, cls)
            except Exception as e:               # the type is what the record keeps
                rec[r["id"] + "__error"] = np.array(type(e).__name__)
                continue
            raise AssertionError("%s: the reference accepts this configuration" % r["id"])
        m, x = model_cases.build_row(r, cls)
        y = m(x, *r.get("fwd_args", ()))
        sd = m.state_dict()
        yf = y.reshape(-1)
        rid = r["id"] + "__"
        rec.update({rid + "y": (yf if yf.numel() <= 257 else yf[sample_index(yf.numel())]).numpy(), rid + "y_shape": np.array(list(y.shape)),
                    rid + "y_sum": np.array(float(yf.double().sum())), rid + "y_abs": np.array(float(yf.double().abs().sum())),
                    rid + "x_sum": np.array(float(x.double().sum())), rid + "p_keys": np.array(list(sd)),
                    rid + "p_sum": np.array([float(v.double().sum()) for v in sd.values()]),
                    rid + "p_abs": np.array([float(v.double().abs().sum()) for v in sd.values()])})
    return rec


def _mhsa_records(mhsa_cases, ref_cls, sample_index, flat_out):
    """mhsa.npz: per row of tests/mhsa_cases.py, built from the reference's class by mhsa_cases.build_row."""
    rec = {"ids": np.array([r["id"] for r in mhsa_cases.ALL_ROWS])}
    for r in mhsa_cases.ALL_ROWS:
        m, x = mhsa_cases.build_row(r, ref_cls(r["mod"], r["cls"]))
        rid = r["id"] + "__"
        if "error" in r:
            try:
                m(x, *mhsa_cases.fwd_args(r))
                rec[rid + "error"] = np.array("")
            except Exception as e:               # the type is what the record keeps
                rec[rid + "error"] = np.array(type(e).__name__)
            continue
        y = flat_out(m(x, *mhsa_cases.fwd_args(r)))
        sd = m.state_dict()
        yf = y.reshape(-1)
        rec.update({rid + "y_samples": yf[sample_index(yf.numel())].numpy(), rid + "y_shape": np.array(list(y.shape)),
                    rid + "y_sum": np.array(float(yf.double().sum())), rid + "y_abs": np.array(float(yf.double().abs().sum())),
                    rid + "x_sum": np.array(float(x.double().sum())), rid + "p_keys": np.array(list(sd)),
                    rid + "p_sum": np.array([float(v.double().sum()) for v in sd.values()]),
                    rid + "p_abs": np.array([float(v.double().abs().sum()) for v in sd.values()])})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    ap.add_argument("--routes-only", action="store_true", help="write tests/golden/live/routes.npz only")
    ap.add_argument("--models-only", action="store_true", help="write tests/golden/live/models.npz only")
    ap.add_argument("--mhsa-only", action="store_true", help="write tests/golden/live/mhsa.npz only")
    args = ap.parse_args()
    ref_root = os.path.abspath(args.ref)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, HERE)
    from make_golden import _stub_timm
    from make_signatures import public_names, shim_modules
    from test_aten_seq_cpu import CASES                      # shapes of the cases (drop-in side; imported before the reference is)
    from route_cases import ROWS, prep_nontrivial
    import model_cases
    import mhsa_cases
    from cases import flat_out, sample_index
    shapes = {c[0]: c[2] for c in CASES}
    # the drop-in package exports the same import paths: forget its modules, then import the reference's
    sys.path.insert(0, os.path.join(ROOT, "pytorch-attention_amd"))
    exported = {name: public_names(importlib.import_module(name)) for name in shim_modules()}
    for k in list(sys.modules):
        if k.split(".")[0] in TOPS:
            del sys.modules[k]
    while os.path.join(ROOT, "pytorch-attention_amd") in sys.path:        # tests/conftest.py put it there too
        sys.path.remove(os.path.join(ROOT, "pytorch-attention_amd"))
    sys.path.insert(0, ref_root)
    _stub_timm()

    def ref_cls(mod, cls):
        m = importlib.import_module(mod)
        assert os.path.abspath(m.__file__).startswith(ref_root), "not the reference's module: %s" % m.__file__
        return getattr(m, cls)

    files = {}
    with torch.no_grad():
        files["mhsa"] = _mhsa_records(mhsa_cases, ref_cls, sample_index, flat_out)
        if args.mhsa_only:
            os.makedirs(os.path.join(HERE, "live"), exist_ok=True)
            np.savez_compressed(os.path.join(HERE, "live", "mhsa.npz"), **files["mhsa"])
            print("wrote mhsa.npz (%d rows)" % len(mhsa_cases.ALL_ROWS))
            return
        files["models"] = _model_records(model_cases, ref_cls, sample_index)
        if args.models_only:
            os.makedirs(os.path.join(HERE, "live"), exist_ok=True)
            np.savez_compressed(os.path.join(HERE, "live", "models.npz"), **files["models"])
            print("wrote models.npz (%d rows)" % len(model_cases.ROWS))
            return
        routes = {"ids": np.array([r["id"] for r in ROWS])}
        for r in ROWS:
            torch.manual_seed(1234)
            m = ref_cls(r["mod"], r["cls"])(*r.get("args", ()), **r.get("kwargs", {})).eval()
            prep_nontrivial(m)
            torch.manual_seed(4321)
            x = torch.randn(*r["shape"])
            y = m(x, *r.get("fwd_args", ()))
            sd = m.state_dict()
            yf = y.reshape(-1)
            routes.update({r["id"] + "__y_samples": yf[sample_index(yf.numel())].numpy(), r["id"] + "__y_shape": np.array(list(y.shape)),
                           r["id"] + "__y_sum": np.array(float(yf.double().sum())), r["id"] + "__y_abs": np.array(float(yf.double().abs().sum())),
                           r["id"] + "__x_sum": np.array(float(x.double().sum())), r["id"] + "__p_keys": np.array(list(sd)),
                           r["id"] + "__p_sum": np.array([float(v.double().sum()) for v in sd.values()]),
                           r["id"] + "__p_abs": np.array([float(v.double().abs().sum()) for v in sd.values()])})
        files["routes"] = routes
        if args.routes_only:
            os.makedirs(os.path.join(HERE, "live"), exist_ok=True)
            np.savez_compressed(os.path.join(HERE, "live", "routes.npz"), **routes)
            print("wrote routes.npz (%d rows)" % len(ROWS))
            return
        for name, (mod, cls, a, kw) in REF_CLASSES.items():
            torch.manual_seed(1234)
            m = ref_cls(mod, cls)(*a, **kw).eval()
            torch.manual_seed(4321)
            x = torch.randn(*shapes[name])
            y = m(x, 6, 6) if name == "xca_block" else m(x)
            sd = m.state_dict()
            files["aten_" + name] = {"y": y.numpy(), "x_sum": np.array(float(x.double().sum())), "p_keys": np.array(list(sd)),
                                     "p_sum": np.array([float(v.double().sum()) for v in sd.values()]),
                                     "p_abs": np.array([float(v.double().abs().sum()) for v in sd.values()])}
        Fourier = ref_cls("vision_transformers.xcit", "PositionalEncodingFourier")
        for H, W, hidden, temp in FOURIER_GRIDS:
            m = Fourier(hidden_dim=hidden, dim=2 * hidden, temperature=temp)
            m.token_projection.weight.copy_(torch.eye(2 * hidden).reshape(2 * hidden, 2 * hidden, 1, 1))
            m.token_projection.bias.zero_()
            files.setdefault("fourier", {})["%dx%dx%dx%d" % (H, W, hidden, temp)] = m(2, H, W)[1].permute(1, 2, 0).reshape(H * W, 2 * hidden).numpy()
        for i, (shape, C, red) in enumerate(CHAN_SHAPES):
            torch.manual_seed(7)
            x = torch.randn(*shape)
            se = ref_cls("attention_mechanisms.se_module", "SELayer")(C, red).eval()
            cb = ref_cls("attention_mechanisms.cbam", "CBAM")(C, red, 3).eval()
            ec = ref_cls("attention_mechanisms.eca", "ECALayer")(C).eval()
            files.setdefault("chan", {}).update({"chan%d__x" % i: x.numpy(), "chan%d__se_w1" % i: se.fc[0].weight.numpy(), "chan%d__se_w2" % i: se.fc[2].weight.numpy(),
                        "chan%d__cbam_w1" % i: cb.ca.fc[0].weight.numpy(), "chan%d__cbam_w2" % i: cb.ca.fc[2].weight.numpy(),
                        "chan%d__cbam_ws" % i: cb.sa.conv.weight.numpy(), "chan%d__eca_w" % i: ec.conv.weight.numpy(),
                        "chan%d__se_y" % i: se(x).numpy(), "chan%d__cbam_y" % i: cb(x).numpy(), "chan%d__eca_y" % i: ec(x).numpy()})
        Lepe = ref_cls("vision_transformers.cswin", "LePEAttention")
        torch.manual_seed(3)
        for i, (reso, idx, split, dim, heads) in enumerate(LEPE_MODES):
            m = Lepe(dim, reso, idx, split_size=split, num_heads=heads).eval()
            qkv = torch.randn(3, 2, reso * reso, dim)
            files.setdefault("lepe", {}).update({"lepe%d__qkv" % i: qkv.numpy(), "lepe%d__w" % i: m.get_v.weight.numpy(), "lepe%d__b" % i: m.get_v.bias.numpy(),
                        "lepe%d__y" % i: m(qkv).numpy()})
    os.makedirs(os.path.join(HERE, "live"), exist_ok=True)
    for fname, arrays in files.items():
        np.savez_compressed(os.path.join(HERE, "live", fname + ".npz"), **arrays)

    names = {}
    for name in exported:
        with contextlib.redirect_stdout(io.StringIO()):          # setr.py runs its smoke block at import time
            ref = importlib.import_module(name)
        assert os.path.abspath(ref.__file__).startswith(ref_root), ref.__file__
        names[name] = sorted(k for k in vars(ref) if not k.startswith("_"))
    with open(os.path.join(HERE, "reference_names.json"), "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
    print("wrote %d files and the public names of %d reference modules" % (len(files), len(names)))


if __name__ == "__main__":
    main()
