"""GPU tests (-m gpu): saturation sweep over the drop-in modules of tests/golden/cases.py.

The drop-in modules promise the reference's numbers at any input or weight scale (include/mi355attn.h fp16 range guard):
every kernel that converts an fp32 value to an fp16 MFMA operand reports a saturation (|v| >= 65520) into the range word, and
range_fallback_forward then re-runs the forward in strict mode.  Each row below stresses one case of the parity table so that some fp16
operand saturates (or, for the vector cases and the LayerNorm-fronted blocks, so that nothing may fall back), and checks

  * the fp64 reference is finite (otherwise the construction is wrong, not the kernel);
  * the fallback fires exactly when the row says so -- one RuntimeWarning -- and never otherwise (a spurious re-run costs 3-7x);
  * the result matches the fp64 reference: 2e-4 after a strict re-run, the case's parity tolerance on the fast path;
  * for a row that fires, the raw fast path (range_fallback = 0) is non-finite or fails the 1e-3 bar -- the stress is real;
  * a second call of the same module returns the same bits.

Perturbations: "x" scales the seeded input so that max|x| = 4 x 65504.  "w:<param>[:<part>]" multiplies one weight (or its v / kv
third or half: "v" = the last third of a fused qkv weight, "v2" = the last half of a fused kv weight) by W_SCALE, so that the tensor
converted right after it passes the fp16 range.  Only value-path weights are scaled: no softmax becomes one-hot.
"""
import importlib
import warnings

import pytest
import torch

from cases import BY_ID, build_case, flat_out, make_arg
from conftest import assert_parity, max_abs_ratio, no_range_fallback, rel_fro

pytestmark = pytest.mark.gpu

FP16_MAX = 65504.0
X_PEAK = 4 * FP16_MAX
W_SCALE = 1.0e6            # init-scale weights x inputs give O(0.1-1) products: x 1e6 puts them far beyond 65520
FIRES_TOL = 2e-4           # the bar of the existing fallback test (test_range_guard_gpu.py)
FALLBACK_MSG = "re-running this forward in strict mode"

VECTOR_ONLY = {"se64", "cbam64", "eca64", "se256", "cbam256", "eca256", "simam64", "srm64", "gctg64", "lct64", "gct64", "gct64_l1",
               "simam256", "srm256", "gctg256", "lct256", "gct256", "se_effnet", "se_mnasnet", "se_mbv3", "se_ghost"}
VECTOR_CHAINS = {"gc64", "coord64", "triplet64", "triplet_k5", "bam64", "gc256", "coord256", "coord_ragged", "triplet256", "bam256",
                 "gc_ragged", "bam_ragged", "triplet_tall", "sk64", "sk256", "sk_ragged", "coord_bigplane", "triplet_bigplane_k9",
                 "bam512", "sk_wide_groups"}
UNSCALED_LOGITS = {"pam64", "pam64_ragged"}        # held to 1e-3 even after a strict re-run (test_gpu_parity.py)

# (case id, perturbation, fallback fires).  Fast-path rows ("does not fire") of the MFMA cases are LayerNorm-fronted blocks whose first
# conversion normalises the scaled input away, and PAM, whose unscaled logits are computed in strict mode whatever the precision.
MFMA_ROWS = [
    ("da64", "x", True), ("da64", "w:convA.weight", True),
    ("vit_attn", "x", True), ("vit_attn", "w:qkv.weight:v", True),
    ("vit_attn_h4", "x", True), ("vit_attn_h4", "w:qkv.weight:v", True),
    ("vit_attn_d128", "x", True), ("vit_attn_d128", "w:qkv.weight:v", True),
    ("vit_attn_d96", "x", True), ("vit_attn_d96", "w:qkv.weight:v", True),
    ("vit_enc", "x", False), ("vit_enc", "w:mlp.fc1.weight", True),
    ("cswin_s1", "x", False), ("cswin_s1", "w:qkv.weight:v", True),
    ("cswin_s2", "x", False), ("cswin_s2", "w:mlp.fc1.weight", True),
    ("cswin_s3", "x", False), ("cswin_s3", "w:qkv.weight:v", True),
    ("cswin_s4", "x", False), ("cswin_s4", "w:mlp.fc1.weight", True),
    ("xca", "x", True), ("xca", "w:qkv.weight:v", True),
    ("xca_block", "x", False), ("xca_block", "w:mlp.fc1.weight", True),
    ("mixer", "x", False), ("mixer", "w:channel_mlp.fc1.weight", True),
    ("xcit_cls_block", "x", False), ("xcit_cls_block", "w:mlp.fc1.weight", True),
    ("xcit_cls_block_tn", "x", False), ("xcit_cls_block_tn", "w:mlp.fc1.weight", True),
    ("pam64", "x", False), ("pam64", "w:d.weight", False),
    ("pam64_ragged", "x", False), ("pam64_ragged", "w:d.weight", False),
    ("cam64", "x", True), ("cam256", "x", True),
    ("setr_attn", "x", True), ("setr_attn", "w:qkv.weight:v", True),
    ("moat_attn", "x", True), ("moat_attn", "w:qkv.weight:v", True),
    ("pvt_attn_s1", "x", True), ("pvt_attn_s1", "w:v.weight", True),
    ("pvt_attn_s3", "x", True), ("pvt_attn_s3", "w:v.weight", True),
    ("cmt_attn", "x", True), ("cmt_attn", "w:v.weight", True),
    ("segformer_attn", "x", True), ("segformer_attn", "w:kv.weight:v2", True),
    ("dilate_gattn", "x", True), ("dilate_gattn", "w:qkv.weight:v", True),
    ("dilate_gattn_d32", "x", True), ("dilate_gattn_d32", "w:qkv.weight:v", True),
    ("bvit_attn", "x", True), ("bvit_attn", "w:to_qkv.weight:v", True),
    ("bvit_attn_d48", "x", True), ("bvit_attn_d48", "w:to_qkv.weight:v", True),
    ("effformer_attn", "x", True), ("effformer_attn", "w:v.weight", True),
    ("kvt_attn", "x", True), ("kvt_attn", "w:qkv.weight:v", True),
    ("kvt_attn_small", "x", True), ("kvt_attn_small", "w:qkv.weight:v", True),
    ("cvt_attn", "x", True), ("cvt_attn", "w:conv_proj_qkv.2.weight:v", True),
    ("cvt_attn_d24", "x", True), ("cvt_attn_d24", "w:conv_proj_qkv.2.weight:v", True),
    ("p2t_attn", "x", True), ("p2t_attn", "w:kv.0.weight:v2", True),
    ("p2t_attn_d40", "x", True), ("p2t_attn_d40", "w:kv.0.weight:v2", True),
    ("se_effnetv2", "x", False), ("se_moat", "x", False),
    # full models at batch 1: vit_full's patch embedding converts raw pixels (im2col16); XCiT's convolutional stem (implicit GEMM)
    ("vit_full", "x", True), ("xcit_nano_full", "x", True),
]
VECTOR_ROWS = [(cid, "x", False) for cid in sorted(VECTOR_ONLY | VECTOR_CHAINS)]
ROWS = MFMA_ROWS + VECTOR_ROWS
FULL_BATCH1 = {"vit_full", "xcit_nano_full"}
# tolerance overrides, with the reason
TOL_OVERRIDE = {cid: (1e-3, "unscaled PAM logits amplify operand rounding even in strict mode") for cid in UNSCALED_LOGITS}
# Rows whose float64 reference is ill-conditioned at this scale: the case's own oracle run in fp32 torch (no MFMA anywhere) already misses
# the row's bar.  The test measures that and xfails the parity check only then (a listed row whose fp32 oracle meets the bar fails); the
# fallback decision is asserted as for every row.
ILL_CONDITIONED = {
    ("bam256", "x"): "1 + sigmoid gates of 1e5-scale BatchNorm outputs (fp32 torch 1.3e-3 off)",
    ("bam64", "x"): "the same gates (fp32 torch 7.4e-4 off)",
    ("se_ghost", "x"): "hard-sigmoid gate near its kinks (fp32 torch 1.9e-4 off)",
    ("p2t_attn", "x"): "pooled 2.6e5-scale tokens into an unnormalised q (fp32 torch 3.5e-3 off)",
}
# Known gaps: the row xfails only while its stated symptom is observed, and fails (to be promoted) once the symptom is gone.
#   "precision": nothing falls back (correctly) and the output is finite, but the fp32 kernel misses its bar where fp32 torch meets it.
#   "strict":  the fallback fires once and returns the strict-mode result, but strict mode itself misses the 2e-4 bar while fp32 torch
#              meets it -- logits ~1e10 with near-tied maxima: the 16-bit-mantissa hi / lo split picks other maxima.
KNOWN_GAPS = {
    ("vit_attn", "x"): ("strict", "strict-mode accuracy at 1e10-scale logits: 0.27 off the float64 reference (fp32 torch 6.5e-7)"),
    ("kvt_attn", "x"): ("strict", "strict-mode accuracy at 1e10-scale logits and a top-k on them: 0.45 off (fp32 torch 7.7e-7)"),
    ("p2t_attn_d40", "x"): ("strict", "strict-mode accuracy on pooled 2.6e5-scale tokens: 1.8e-3 off (fp32 torch 9.9e-5)"),
    ("se_mbv3", "x"): ("precision", "fp32 vector kernel at 2.6e5 scale: 1.2e-5 off against the 1e-5 bar (fp32 torch 6.4e-6)"),
}


def row_id(row):
    return f"{row[0]}-{row[1]}"


def fast_tol(cid):
    return 1e-5 if cid in VECTOR_ONLY else (3e-5 if cid in VECTOR_CHAINS else 1e-3)


def row_tol(row):
    cid, pert, fires = row
    if cid in TOL_OVERRIDE:
        return TOL_OVERRIDE[cid][0]
    return FIRES_TOL if fires else fast_tol(cid)


def _perturb(m, x, pert):
    """Apply a perturbation in place to the CPU module / input; returns the (possibly new) input."""
    if pert == "x":
        return x * (X_PEAK / float(x.abs().max()))
    assert pert.startswith("w:"), pert
    parts = pert[2:].split(":")
    p = dict(m.named_parameters())[parts[0]]
    with torch.no_grad():
        if len(parts) == 1:
            p.mul_(W_SCALE)
        elif parts[1] == "v":                                  # last third of a fused (q, k, v) output dimension
            p[2 * p.shape[0] // 3:].mul_(W_SCALE)
        elif parts[1] == "v2":                                 # last half of a fused (k, v) output dimension
            p[p.shape[0] // 2:].mul_(W_SCALE)
        else:
            raise ValueError(pert)
    return x


def build_row(row):
    """(cpu module, cpu input, forward args) of a row: the case under the seed protocol, perturbed."""
    cid, pert, _ = row
    c = BY_ID[cid]
    cls = getattr(importlib.import_module(c["mod"]), c["cls"])
    m, x = build_case(c, cls)
    if cid in FULL_BATCH1:
        x = x[:1].contiguous()
    x = _perturb(m, x, pert)
    args = [make_arg(a) for a in c.get("fwd_args", ())]
    return m, x, args


def reference(row, m, x):
    """The case's oracle in float64 on the CPU, state dict cast to float64."""
    c = BY_ID[row[0]]
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in m.state_dict().items()}
    ref = flat_out(c["oracle"](x.double(), sd, torch.float64))
    return ref.double()


def _call(dev, x, args):
    dargs = [a.cuda() if isinstance(a, (torch.Tensor, torch.nn.Module)) else a for a in args]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = flat_out(dev(x, *dargs))
        torch.cuda.synchronize()
    return y, [str(i.message) for i in w if FALLBACK_MSG in str(i.message)]


class _raw_fast_path(no_range_fallback):
    """The fp16 fast path with the range machinery out of the way: no re-run, and no pre-launch range check inside the forward either
    (with range_fallback = 0 a later launch of the same forward would raise on an earlier launch's report)."""

    def __enter__(self):
        from mi355attn import functional
        self.fn = functional._range_check
        functional._range_check = lambda: None
        return super().__enter__()

    def __exit__(self, *exc):
        from mi355attn import functional
        functional._range_check = self.fn
        return super().__exit__(*exc)


def _strict(dev, x, args):
    """The module run explicitly in strict mode (what a re-run computes)."""
    from mi355attn import functional
    with functional._forced_strict(dev):
        y, hits = _call(dev, x, args)
    assert not hits
    return y


def _settle():
    import mi355attn
    try:
        mi355attn.range_status(wait=True)
    except mi355attn.Mi355RangeError:
        pass


_REF_CACHE = {}


def _fp32_oracle_error(row, m, x, ref):
    c = BY_ID[row[0]]
    r32 = flat_out(c["oracle"](x, m.state_dict(), torch.float32))
    return max(rel_fro(r32, ref), max_abs_ratio(r32, ref))


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_saturation_falls_back_exactly_when_fp16_saturates(row):
    import mi355attn
    cid, pert, fires = row
    m, x, args = build_row(row)
    key = (cid, pert)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = reference(row, m, x)
    ref = _REF_CACHE[key]
    assert torch.isfinite(ref).all(), f"{cid} {pert}: the fp64 reference is not finite -- the construction is wrong, not the kernel"
    dev, xd = m.cuda(), x.cuda()
    _settle()
    try:
        if fires:                                              # the stress is real: the raw fp16 fast path is wrong without the fallback
            with _raw_fast_path():
                y_raw, _ = _call(dev, xd, args)
            _settle()
            y_raw = y_raw.cpu()
            if torch.isfinite(y_raw).all():
                with pytest.raises(AssertionError):
                    assert_parity(y_raw, ref, 1e-3, f"{cid} {pert} [raw fast path]")
        assert mi355attn.get_option("range_fallback") == 1, "the default"
        y, hits = _call(dev, xd, args)
        if fires:
            assert len(hits) == 1, f"{cid} {pert}: expected one strict re-run, got {hits}"
        else:
            assert not hits, f"{cid} {pert}: spurious strict re-run: {hits}"
        if fires:
            assert torch.equal(y, _strict(dev, xd, args)), f"{cid} {pert}: the re-run differs from the module in strict mode"
        y2, _ = _call(dev, xd, args)
        assert torch.equal(y, y2), f"{cid} {pert}: a second call differs"
        tol, what = row_tol(row), f"{cid} {pert} [{'strict re-run' if fires else 'fast path'}]"
        gap = KNOWN_GAPS.get(key)
        if key in ILL_CONDITIONED or gap:
            e32 = _fp32_oracle_error(row, m, x, ref)
            try:
                assert_parity(y.cpu(), ref, tol, what)
            except AssertionError:
                if key in ILL_CONDITIONED:
                    assert e32 > tol, f"{what}: listed as ill-conditioned, but fp32 torch is {e32:.2e} off, inside the {tol:g} bar"
                    pytest.xfail(f"ill-conditioned reference: {ILL_CONDITIONED[key]}")
                assert e32 <= tol and torch.isfinite(y).all(), f"{what}: not the stated gap ({gap[1]})"
                pytest.xfail(gap[1])
            pytest.fail(f"{what}: {'ill-conditioned' if key in ILL_CONDITIONED else 'gap'} row now meets its bar: promote it")
        assert_parity(y.cpu(), ref, tol, what)
    finally:
        _settle()                                              # range_status(wait=True): nothing pending for the next test


def test_fallback_raises_a_hip_error_of_the_wait_instead_of_re_running():
    """range_fallback_forward re-runs only on MI355_ERANGE: any other code of mi355_range_wait (here MI355_EHIP) is raised, not
    mistaken for an overflow."""
    import mi355attn
    from mi355attn import _ffi, functional
    m, x, args = build_row(("moat_attn", "w:qkv.weight:v", True))
    dev, xd = m.cuda(), x.cuda()
    real = functional.lib()

    class Proxy:
        def __getattr__(self, name):
            if name == "mi355_range_wait":
                return lambda: -3                              # MI355_EHIP
            return getattr(real, name)

    _settle()
    old = functional.lib
    functional.lib = lambda: Proxy()
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with pytest.raises(_ffi.Mi355Error) as e, torch.no_grad():
                dev(xd, *args)
        assert not isinstance(e.value, mi355attn.Mi355RangeError)
        assert not [i for i in w if FALLBACK_MSG in str(i.message)]
    finally:
        functional.lib = old
        _settle()


def test_fused_mlp_rejects_a_flag_word_outside_0_to_3():
    """mi355_mlp_fused_fwd / mi355_proj_mlp_fused_fwd: `layernorm` is a flag word (bit 0 LayerNorm, bit 1 range proven); anything else
    is MI355_EINVAL before a launch."""
    from mi355attn import _ffi
    lib = _ffi.lib()
    t = torch.zeros(64 * 256, device="cuda")
    p = t.data_ptr()
    for flag in (4, -1, 7):
        assert lib.mi355_mlp_fused_fwd(p, p, p, p, p, p, p, 64, 64, 256, flag, 1e-5, 1, None) == -1
        assert lib.mi355_proj_mlp_fused_fwd(p, p, p, p, p, p, p, p, p, p, 64, 64, 256, flag, 1e-5, 1, None) == -1


@pytest.mark.parametrize("which", ["input", "output"])
def test_linear16_x32_leaves_the_code_of_cast16_then_linear16(which):
    """mi355_linear16_x32_fwd (the fp32 -> 16-bit cast inside the GEMM staging) leaves the same range code as the cast16 + linear16
    sequence it replaces: code 1 when the input saturates, code 3 when only the output does."""
    import mi355attn
    from mi355attn import _ffi, functional as F
    M, N, K = 50176, 1152, 384                                # XCA's qkv product at B = 256 (xcit.py:251), with GELU
    g = torch.Generator().manual_seed(5)
    if which == "input":
        x = torch.randn(M, K, generator=g)
        x[7, 11] = 1.0e5                                       # one input value beyond the fp16 range; its row's outputs are +-inf
        w = torch.randn(N, K, generator=g) * 0.05
    else:
        x = torch.full((M, K), 300.0)                          # fits fp16; every output is gelu(300 * 384) = 115200 > 65520
        w = torch.ones(N, K)
    xd, wd = x.cuda(), w.cuda()
    w16 = F.cast16(wd, 1)

    def code_of(run):
        _settle()
        run()
        torch.cuda.synchronize()
        with pytest.raises(mi355attn.Mi355RangeError) as e:
            mi355attn.range_status(wait=True)
        return str(e.value).split(" converted")[0].split("launch of ")[-1]

    def fused():
        y = torch.empty(M, N, dtype=torch.float16, device="cuda")
        rc = _ffi.lib().mi355_linear16_x32_fwd(_ffi.dptr(xd), _ffi.dptr(w16), None, _ffi.dptr(y), M, N, K, K, N, 1, 1,
                                               _ffi.stream_ptr(xd.device))
        assert rc == 0, "mi355_linear16_x32_fwd takes this shape"

    def two_launch():
        x16 = F.cast16(xd, 1)
        lib = _ffi.lib()
        y = torch.empty(M, N, dtype=torch.float16, device="cuda")
        _ffi.check(lib.mi355_linear16_fwd(_ffi.dptr(x16), _ffi.dptr(w16), None, None, None, _ffi.dptr(y), M, N, K, K, N, 1, 1, 1,
                                          _ffi.stream_ptr(xd.device)), "mi355_linear16_fwd")

    a, b = code_of(fused), code_of(two_launch)
    assert a == b, (a, b)
    assert ("mi355_cast16_fwd" in a) == (which == "input"), a
    _settle()
