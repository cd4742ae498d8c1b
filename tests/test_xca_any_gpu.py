"""GPU tests (-m gpu): XCiT on any head width -- xca_any_kernel (csrc/xcit.hip) behind mi355_xca_fwd / mi355_xca16_fwd and
class_attn_any_kernel (csrc/cls_attn.hip) behind mi355_class_attn_fwd, for every head width from 1 to 256 that has no template kernel.
The shapes are tests/xca_any_cases.py; every case is a few thousand elements.

Bars
  fp32 -> fp32        assert_parity at 2e-5, what tests/test_ops_gpu.py::test_xca_core holds the template kernels to.
  16-bit output       every element: |got - ref| <= u |ref| + 2e-5 max|ref| (+ 2^-25 absolute below the fp16 normal range), u = 2^-11 for
                      fp16 and 2^-8 for bf16: one rounding at the store on top of the fp32-class result (the form of tests/io16_common.py).
                      With a 16-bit qkv the reference is computed from the rounded tensor (the widening at the load is exact).
  class attention     2e-6, the bar of test_class_attention_core.
  modules             TOL of tests/test_routes_gpu.py (1e-3 at precision 1, 5e-5 strict) against the fp64 oracle.
"""
import importlib

import pytest
import torch

import xca_any_cases as X
from conftest import assert_parity
from io16_common import U
from test_ops_gpu import F, _xca_core_ref
from test_routes_gpu import TOL, _run

pytestmark = pytest.mark.gpu

MODES = ["f32", "f32_to_f16", "f32_to_bf16", "f16", "bf16"]      # fp32 -> fp32, fp32 -> 16 bit, 16 bit -> same
_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
_REFS = {}


def _qkv(case, seed_off=0):
    B, N, h, d = case
    g = torch.Generator().manual_seed(1000 * d + N + seed_off)
    return torch.randn(B, N, 3 * h * d, generator=g), torch.rand(h, generator=g) + 0.5


def _mode(mode):
    """(dtype of qkv or None for fp32, dtype of the output or None for fp32)."""
    if mode == "f32":
        return None, None
    dt = _DT[mode.rsplit("_", 1)[-1]]
    return (None if mode.startswith("f32_to") else dt), dt


def _core(qkv, temp, h, mode):
    """Run the core in `mode`: (output, the qkv tensor the kernel saw as fp64)."""
    din, dout = _mode(mode)
    x = qkv if din is None else qkv.to(din)
    if dout is None:
        out = F().xca_core(x.cuda(), temp.cuda(), h)
    else:
        out = F().xca_core(x.cuda(), temp.cuda(), h, precision=1 if dout == torch.float16 else 2, out16=True)
        assert out.dtype == dout
    return out.cpu(), x.double()


def _ref(key, seen, temp, h):
    """fp64 reference, computed once per (case, input rounding)."""
    if key not in _REFS:
        _REFS[key] = _xca_core_ref(seen, temp.double(), h)
    return _REFS[key]


def _check(out, ref, mode, what):
    _, dout = _mode(mode)
    if dout is None:
        rf, ma = assert_parity(out, ref.float(), 2e-5, what)
        print(f"[xca_any] {what}: rel_fro {rf:.2e} max_abs_ratio {ma:.2e}")
        return
    got, ref = out.double(), ref.double()
    assert torch.isfinite(got).all(), what
    bound = U[dout] * ref.abs() + 2e-5 * float(ref.abs().max())
    if dout == torch.float16:
        bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
    worst = float(((got - ref).abs() / bound).max())
    print(f"[xca_any] {what}: max err / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", X.CORE, ids=lambda c: "x".join(map(str, c)))
def test_core_matches_fp64(case, mode):
    B, N, h, d = case
    qkv, temp = _qkv(case)
    out, seen = _core(qkv, temp, h, mode)
    _check(out, _ref((case, _mode(mode)[0]), seen, temp, h), mode, f"xca_any{case} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", X.MASK, ids=lambda c: "x".join(map(str, c)))
def test_padded_columns_are_masked(case, mode):
    """k = -q at temperature 10: every diagonal logit is -10, a padded column left at logit 0 would take almost the whole row."""
    B, N, h, d = case
    qkv, _ = _qkv(case, 7)
    C = h * d
    qkv[:, :, C:2 * C] = -qkv[:, :, :C]
    temp = torch.full((h,), X.MASK_TEMPERATURE)
    out, seen = _core(qkv, temp, h, mode)
    _check(out, _xca_core_ref(seen, temp.double(), h), mode, f"mask{case} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_zero_channel_takes_the_clamp(mode):
    """One all-zero q channel: its norm is clamped at 1e-12, its logits are 0 and its row of A is uniform over the d live columns."""
    B, N, h, d = X.ZERO_CHANNEL
    qkv, temp = _qkv(X.ZERO_CHANNEL, 11)
    qkv[:, :, d + 3] = 0.0                                  # channel 3 of head 1 of q
    out, seen = _core(qkv, temp, h, mode)
    ref = _xca_core_ref(seen, temp.double(), h)
    _check(out, ref, mode, f"zero channel {mode}")
    v = seen[:, :, 2 * h * d + d:2 * h * d + 2 * d]
    assert torch.allclose(ref[:, :, d + 3], v.mean(-1), rtol=1e-12, atol=1e-12)      # the reference row is the mean of the head's v channels


@pytest.mark.parametrize("mode", ["f32", "f32_to_f16", "bf16"])
@pytest.mark.parametrize("case", [(2, 70, 3, 5), (2, 33, 2, 72), (1, 64, 1, 256)], ids=lambda c: "x".join(map(str, c)))
def test_two_runs_are_bit_equal(case, mode):
    qkv, temp = _qkv(case)
    a, _ = _core(qkv, temp, case[2], mode)
    b, _ = _core(qkv, temp, case[2], mode)
    assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("case", X.BATCH_INDEPENDENCE, ids=lambda c: "x".join(map(str, c)))
def test_an_image_does_not_depend_on_its_batch(case, mode):
    qkv, temp = _qkv(case)
    whole, _ = _core(qkv, temp, case[2], mode)
    alone, _ = _core(qkv[1:2].contiguous(), temp, case[2], mode)
    assert torch.equal(whole[1:2], alone)


def _tags(fn):
    import mi355attn
    return [r[0] for r in mi355attn.kernel_trace(fn)]


@pytest.mark.parametrize("mode", ["f32", "f32_to_f16", "f16"])
def test_routing(mode):
    from mi355attn._ffi import Mi355Error
    for d in X.ROUTING_TEMPLATE:
        qkv, temp = _qkv((1, 20, 2, d))
        tags = _tags(lambda: _core(qkv, temp, 2, mode))
        assert any(t.startswith(("xca_kernel<", "xca_tr_kernel<")) for t in tags) and not any("xca_any_kernel" in t for t in tags), tags
    for d in X.ROUTING_ANY:
        qkv, temp = _qkv((1, 20, 2, d))
        tags = _tags(lambda: _core(qkv, temp, 2, mode))
        din, dout = _mode(mode)
        want = f"xca_any_kernel<d={d}" + (",in16" if din is not None else "") + (",out16" if dout is not None else "") + ">"
        assert any(t.startswith(want) for t in tags), (want, tags)
    qkv, temp = _qkv((1, 4, 1, X.ROUTING_REFUSED))
    with pytest.raises(Mi355Error):
        _core(qkv, temp, 1, mode)


@pytest.mark.parametrize("case", X.CLASS_ATTN, ids=lambda c: "x".join(map(str, c)))
def test_class_attention_matches_fp64(case):
    """One query per (image, head) against fp64; q / k / v are consumed in place from the fused (B, N, 3C) projection."""
    B, N, h, d = case
    torch.manual_seed(N + d)
    C = h * d
    qkv = torch.randn(B, N, 3 * C)
    scale = d ** -0.5
    q = qkv[:, 0, :C].double().reshape(B, h, 1, d)
    k = qkv[:, :, C:2 * C].double().reshape(B, N, h, d).permute(0, 2, 1, 3)
    v = qkv[:, :, 2 * C:].double().reshape(B, N, h, d).permute(0, 2, 1, 3)
    a = torch.softmax((q * k).sum(-1) * scale, dim=-1)
    ref = (a.unsqueeze(2) @ v).transpose(1, 2).reshape(B, C)
    dev = qkv.cuda()
    out = []
    tags = _tags(lambda: out.append(F().class_attention(dev[:, 0, :C], dev[:, :, C:2 * C], dev[:, :, 2 * C:], h, scale, N, N * 3 * C, 3 * C)))
    assert any(t.startswith(f"class_attn_any_kernel<d={d}") for t in tags), tags
    assert_parity(out[0].cpu(), ref.float(), 2e-6, f"class attention {case}")


_BUILT = {}


def _built(rid):
    """(state dict, input, fp64 reference) of a module row: built once, shared by both precisions."""
    if rid not in _BUILT:
        row = X.MODULES[rid]
        m, x = X.build(rid)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _BUILT[rid] = (sd, x, row["oracle"](x, sd, torch.float64).float())
    return _BUILT[rid]


@pytest.mark.parametrize("prec", [1, 0])
@pytest.mark.parametrize("rid", list(X.MODULES))
def test_module_matches_fp64(rid, prec):
    row = X.MODULES[rid]
    sd, x, ref = _built(rid)
    m = getattr(importlib.import_module(X._XCIT), row["cls"])(*row.get("args", ()), **row["kwargs"]).eval()
    m.load_state_dict(sd)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = prec
    y, tags, fired = _run(m.cuda(), x.cuda(), row.get("fwd_args", ()))
    assert not fired, f"{rid} p{prec}: range fallback fired: {fired}"
    d = row["d"]
    if row["cls"] != "ClassAttentionBlock":
        assert any(t.startswith(f"xca_any_kernel<d={d}") for t in tags), tags
    if row["cls"] in ("ClassAttentionBlock", "XCiT"):
        assert any(t.startswith(f"class_attn_any_kernel<d={d}") for t in tags), tags
    if row.get("in16") and prec == 1:
        assert any(t.startswith(f"xca_any_kernel<d={d},in16,out16>") for t in tags), tags
    assert_parity(y.cpu(), ref, TOL[prec], f"{rid} p{prec}")
