"""GPU tests (-m gpu): reports of the fp16 range word and the exchange-failure word belong to the thread that launched.

module(x) promises the fp32 reference's numbers at any scale (range_fallback_forward: arm, wait for the forward's last fp16 producer,
re-run in strict mode when the range word fired).  These cases run two threads on one device, each on its own stream, and order every
step with barriers and stream synchronisation, so that each case is deterministic and does not depend on timing:

  * C ABI, range word: A's saturated producer (cast16 / an fp32-input GEMM / the fp32-I/O attention core) is never seen -- let alone
    cleared -- by B's mi355_range_wait / mi355_range_status, and A's own wait reports it exactly once.
  * C ABI, no arm (range_fallback = 0): A's saturation is reported by A's next call, never by B's.
  * exchange-failure word: A's poll time-out does not fail B's sync_status or B's SE launch; A's sync_status reports it.
  * modules against float64: A forwards a saturating input (one strict re-run per forward), B a clean one on its own module or on the
    same module (never a re-run, bit-identical to its fp16 solo run), ten forwards each, starts aligned by a barrier.
"""
import threading
import traceback
import warnings

import pytest
import torch

import oracle as O
from cases import BY_ID, flat_out
from conftest import assert_parity, no_range_fallback
from test_range_sweep_gpu import FIRES_TOL, build_row, reference

pytestmark = pytest.mark.gpu

BARRIER_S = 60.0           # a step that takes longer than this is broken, not slow: the barrier breaks and the case fails
JOIN_S = 120.0
ITERS = 10
FAST_TOL = 1e-3            # the MFMA cases' parity bar (test_gpu_parity.py)
MI355_OK, MI355_ERANGE = 0, -5


def _run_threads(*fns):
    """Run fn(barrier) for each fn on its own thread; re-raise the first failure (with its traceback) on the calling thread."""
    bar = threading.Barrier(len(fns), timeout=BARRIER_S)
    out, errors = [None] * len(fns), []

    def wrap(i, fn):
        try:
            out[i] = fn(bar)
        except BaseException:                                  # noqa: BLE001 -- pytest.fail / AssertionError alike
            errors.append(f"thread {'AB'[i] if i < 2 else i}:\n{traceback.format_exc()}")
            bar.abort()

    ts = [threading.Thread(target=wrap, args=(i, fn), daemon=True) for i, fn in enumerate(fns)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in ts), "a thread did not finish"
    if errors:
        pytest.fail("\n".join(errors), pytrace=False)
    return out


def _settle():
    import mi355attn
    torch.cuda.synchronize()
    for check in (mi355attn.range_status, mi355attn.sync_status):
        try:
            check()
        except mi355attn.Mi355Error:
            pass


def _last_error():
    from mi355attn import _ffi
    msg = _ffi.lib().mi355_last_error()
    return msg.decode() if msg else ""


# ---- C ABI: the range word --------------------------------------------------------------------------------------------------
# producer -> (its inputs, clean or with one value of 1e6; the launch; a piece of the text its code produces)
def _producer(kind, dirty):
    from mi355attn import _ffi
    from mi355attn._ffi import dptr
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(17)
    if kind == "cast16":
        x = torch.randn(4096, generator=g)
        if dirty:
            x[123] = 1.0e6
        x = x.cuda()
        y = torch.empty(4096, dtype=torch.float16, device="cuda")
        return lambda: lib.mi355_cast16_fwd(dptr(x), dptr(y), x.numel(), 1, _ffi.stream_ptr(x.device)), "mi355_cast16_fwd"
    if kind == "gemm":                                         # the qkv product of ViT-Base at B = 2, fp32 input (code 6)
        M, N, K = 394, 2304, 768
        x = torch.randn(M, K, generator=g)
        if dirty:
            x[5, 7] = 1.0e6
        x, w = x.cuda(), (0.02 * torch.randn(N, K, generator=g)).cuda()
        y = torch.empty(M, N, device="cuda")
        return (lambda: lib.mi355_linear_fwd(dptr(x), dptr(w), None, None, None, dptr(y), M, N, K, K, N, 0, 1,
                                             _ffi.stream_ptr(x.device)), "fp32-input GEMM")
    assert kind == "sdpa"                                      # the fp32-I/O attention core at precision 1 (code 7)
    B, N, H, d = 2, 197, 12, 64
    qkv = torch.randn(B, N, 3 * H * d, generator=g)
    if dirty:
        qkv[0, 3, 2 * H * d + 5] = 1.0e6                       # a value of v
    qkv = qkv.cuda()
    out = torch.empty(B, N, H * d, device="cuda")
    return (lambda: lib.mi355_sdpa_fwd(dptr(qkv), dptr(out), B, N, H, d, d ** -0.5, 1, _ffi.stream_ptr(qkv.device)),
            "fp32-I/O attention core")


@pytest.mark.parametrize("kind", ["cast16", "gemm", "sdpa"])
def test_range_wait_reports_only_the_calling_threads_launches(kind):
    from mi355attn import _ffi
    lib = _ffi.lib()
    launch_a, what = _producer(kind, True)
    launch_b, _ = _producer(kind, False)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    _settle()

    def a(bar):
        with torch.cuda.stream(sa):
            try:
                assert lib.mi355_range_arm(1) == MI355_OK
                assert launch_a() == MI355_OK, _last_error()
                sa.synchronize()                               # the report is in the word before B looks
                bar.wait()                                     # 1: A's producer has run
                bar.wait()                                     # 2: B has waited and read its status
                rc = lib.mi355_range_wait()
                assert rc == MI355_ERANGE, f"A's own saturation was not reported to A (rc {rc})"
                assert what in _last_error(), _last_error()
                assert lib.mi355_range_wait() == MI355_OK, "reported twice"
                assert lib.mi355_range_status() == MI355_OK
            finally:
                lib.mi355_range_arm(0)

    def b(bar):
        with torch.cuda.stream(sb):
            try:
                bar.wait()                                     # 1
                assert lib.mi355_range_arm(1) == MI355_OK
                assert launch_b() == MI355_OK, _last_error()
                rc = lib.mi355_range_wait()
                assert rc == MI355_OK, f"B's clean {kind} got another thread's report (rc {rc}: {_last_error()})"
                assert lib.mi355_range_status() == MI355_OK, f"B's status holds another thread's report: {_last_error()}"
            finally:
                lib.mi355_range_arm(0)
                bar.wait()                                     # 2

    try:
        _run_threads(a, b)
    finally:
        _settle()


def test_unarmed_saturation_is_reported_by_the_launching_threads_next_call():
    """range_fallback = 0 (the round-3 contract): A's saturated cast is reported by A's next call -- here the pre-launch check of
    the binding's cast16 -- and by no call of B."""
    import mi355attn
    from mi355attn import _ffi, functional as F
    lib = _ffi.lib()
    launch_a, _ = _producer("cast16", True)
    xb = torch.randn(4096, generator=torch.Generator().manual_seed(3)).cuda()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    _settle()

    def a(bar):
        with torch.cuda.stream(sa):
            assert launch_a() == MI355_OK, _last_error()
            sa.synchronize()
            bar.wait()                                         # 1: A's report is in the word
            bar.wait()                                         # 2: B has made its calls
            with pytest.raises(mi355attn.Mi355RangeError, match="mi355_cast16_fwd"):
                F.cast16(xb, 1)
            assert lib.mi355_range_status() == MI355_OK, "reported twice"

    def b(bar):
        with torch.cuda.stream(sb):
            try:
                bar.wait()                                     # 1
                y = F.cast16(xb, 1)                            # its pre-launch check reads B's word only
                sb.synchronize()
                assert torch.isfinite(y).all()
                assert lib.mi355_range_status() == MI355_OK, f"B sees another thread's report: {_last_error()}"
                mi355attn.range_status()
            finally:
                bar.wait()                                     # 2

    try:
        with no_range_fallback():
            _run_threads(a, b)
    finally:
        _settle()


# ---- the exchange-failure word ----------------------------------------------------------------------------------------------
def test_poll_timeout_is_reported_only_to_the_launching_thread():
    """A: one SE launch with a zero poll budget (test_boundary_gpu.py's mechanism), stream synchronised, budget restored.  B then
    sees a clean sync_status and runs the same SE module correctly; A's sync_status reports the time-out afterwards."""
    import mi355attn
    from mi355attn import functional as F
    from mi355attn.modules import SELayer
    torch.manual_seed(1234)
    se = SELayer(256, 16).eval().cuda()
    torch.manual_seed(5)
    x = torch.randn(64, 256, 56, 56, device="cuda")
    xb = x[:3].contiguous()
    ref = O.se_forward(xb.cpu(), se.fc[0].weight.detach().cpu(), se.fc[2].weight.detach().cpu())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    _settle()

    def a(bar):
        with torch.cuda.stream(sa):
            post = F._sync_check
            F._sync_check = lambda: None                       # no post-launch check: the report stays in the word (B is parked)
            try:
                with mi355attn.options(spin_limit=0), torch.no_grad():
                    se(x)
                    sa.synchronize()
            finally:
                F._sync_check = post
            bar.wait()                                         # 1: A's failed exchange has run
            bar.wait()                                         # 2: B is done
            with pytest.raises(mi355attn.Mi355Error, match=r"code -4\).*poll budget"):
                mi355attn.sync_status()
            mi355attn.sync_status()                            # reported once

    def b(bar):
        with torch.cuda.stream(sb):
            try:
                bar.wait()                                     # 1
                mi355attn.sync_status()                        # nothing of B's is pending
                with torch.no_grad():
                    y = se(xb)
                sb.synchronize()
                mi355attn.sync_status()
                return y.cpu()
            finally:
                bar.wait()                                     # 2

    try:
        _, y = _run_threads(a, b)
    finally:
        _settle()
    assert_parity(y, ref, 1e-5, "B's SE launch next to A's reported time-out")


# ---- drop-in modules against float64 ----------------------------------------------------------------------------------------
class _CountStrict:
    """functional._forced_strict, counting the strict re-runs of each thread (warnings capture is process-global, so it cannot)."""

    def __init__(self):
        from mi355attn import functional
        self.functional, self.real = functional, functional._forced_strict
        self.lock, self.by_thread = threading.Lock(), {}

    def __call__(self, *args, **kwargs):
        with self.lock:
            k = threading.get_ident()
            self.by_thread[k] = self.by_thread.get(k, 0) + 1
        return self.real(*args, **kwargs)

    def of_this_thread(self):
        with self.lock:
            return self.by_thread.get(threading.get_ident(), 0)

    def __enter__(self):
        self.functional._forced_strict = self
        return self

    def __exit__(self, *exc):
        self.functional._forced_strict = self.real
        return False


def _forward(m, x):
    with torch.no_grad():
        y = flat_out(m(x))
    torch.cuda.current_stream().synchronize()
    return y.cpu()


def _clean_case(case):
    """A case's module and input under the seed protocol, unperturbed."""
    import importlib
    from cases import build_case
    c = BY_ID[case]
    return build_case(c, getattr(importlib.import_module(c["mod"]), c["cls"]))


# (case, shared module).  Own modules: A's is the sweep row "w:qkv.weight:v" (the value third of qkv x 1e6) on the seeded input, B's
# the unscaled module on the same input.  Shared: one module; A's input is the sweep row "x" (max|x| = 4 x 65504), B's the seeded
# input.  vit_attn runs at (2, 197, 768), ViT-Base; its "x" row is a known strict-mode gap of the sweep, so the shared case uses
# vit_attn_d128, whose "x" row meets the strict bar.
MODULE_CASES = [("vit_attn", False), ("cswin_s3", False), ("vit_attn_d128", True)]


def _module_case(case, shared):
    if shared:
        ma, xa, _ = build_row((case, "x", True))
        mb, xb = ma, _clean_case(case)[1]
    else:
        ma, xa, _ = build_row((case, "w:qkv.weight:v", True))
        mb, xb = _clean_case(case)
    if case == "vit_attn":
        xa, xb = xa[:2].contiguous(), xb[:2].contiguous()
    row = (case, None, None)
    ref_a, ref_b = reference(row, ma, xa), reference(row, mb, xb)
    assert torch.isfinite(ref_a).all() and torch.isfinite(ref_b).all()
    ma = ma.cuda()
    mb = ma if shared else mb.cuda()
    return ma, xa.cuda(), mb, xb.cuda(), ref_a, ref_b


@pytest.mark.parametrize("case,shared", MODULE_CASES, ids=[f"{c}-{'shared' if s else 'own'}" for c, s in MODULE_CASES])
def test_concurrent_forwards_match_float64(case, shared):
    """Ten forwards per thread, starts aligned by a barrier: A's saturate (one strict re-run each, finite, within the strict bar of
    float64, bit-identical to A's solo run), B's do not (no re-run, within 1e-3 of float64, bit-identical to B's solo fp16 run)."""
    import mi355attn
    ma, xa, mb, xb, ref_a, ref_b = _module_case(case, shared)
    assert mi355attn.get_option("range_fallback") == 1, "the default"
    assert mi355attn.default_precision() == mi355attn.PREC_FP16
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    _settle()
    with warnings.catch_warnings(), _CountStrict() as counter:
        warnings.simplefilter("ignore", RuntimeWarning)        # the re-run's warning; counted through _forced_strict instead
        solo_a = _forward(ma, xa)
        assert counter.of_this_thread() == 1, "A's input does not make the solo forward re-run: the stress is not real"
        solo_b = _forward(mb, xb)
        assert counter.of_this_thread() == 1, "B's clean input re-ran on its own"
        assert torch.isfinite(solo_a).all() and torch.isfinite(solo_b).all()
        assert_parity(solo_a, ref_a, FIRES_TOL, f"{case} A solo [strict re-run]")
        assert_parity(solo_b, ref_b, FAST_TOL, f"{case} B solo [fast path]")

        def run(m, x, stream):
            def body(bar):
                ys, reruns = [], []
                with torch.cuda.stream(stream):
                    for _ in range(ITERS):
                        bar.wait()
                        before = counter.of_this_thread()
                        ys.append(_forward(m, x))
                        reruns.append(counter.of_this_thread() - before)
                return ys, reruns
            return body

        (ys_a, runs_a), (ys_b, runs_b) = _run_threads(run(ma, xa, sa), run(mb, xb, sb))
    _settle()
    assert runs_a == [1] * ITERS, f"{case}: A's strict re-runs per forward: {runs_a}"
    assert runs_b == [0] * ITERS, f"{case}: B re-ran in strict mode (another thread's report?): {runs_b}"
    for i, (ya, yb) in enumerate(zip(ys_a, ys_b)):
        assert_parity(ya, ref_a, FIRES_TOL, f"{case} A forward {i} [strict re-run]")
        assert torch.equal(ya, solo_a), f"{case}: A's forward {i} differs from A's solo run"
        assert_parity(yb, ref_b, FAST_TOL, f"{case} B forward {i} [fast path]")
        assert torch.equal(yb, solo_b), f"{case}: B's forward {i} differs from B's solo fp16 run"
    assert mi355attn.default_precision() == mi355attn.PREC_FP16
