"""What the GPU tests of the 16-bit activation paths share (test_io16_gpu.py, test_zoo_io16_gpu.py, test_axis_io16_gpu.py,
test_da_io16_gpu.py): the two I/O types, their unit roundoff and precision codes, the seeded input, distances in representable
values, the status words and a traced forward.  A plain module, not a test file: nothing here is collected."""
import torch

DTYPES = [torch.float16, torch.bfloat16]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}            # half an ulp, relative
IO = {torch.float16: 1, torch.bfloat16: 2}                            # the `io` argument of the *16 entries


def _input(shape, dtype, seed=4321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _check_chan(got, ref, dtype, what):
    """The bound of the channel gates (test_io16_gpu.py, test_zoo_io16_gpu.py: u |ref| + 1e-5 max|ref|), every element; prints the figures
    before it asserts.  test_axis_io16_gpu.py has its own _check with the axis gates' fp32 allowance."""
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), what
    got, ref = got.detach().cpu().double(), ref.double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs from the reference"
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), f"{what}: inf pattern"
    t32 = 1e-5 * float(ref[fin].abs().max()) if fin.any() else 0.0
    bound = U[dtype] * ref.abs() + t32
    if dtype == torch.float16:
        bound = bound + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
    err = (got - ref).abs()
    worst = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    print(f"[io16] {what}: max err / bound = {worst:.3f}, max abs err = {float(err[fin].max()) if fin.any() else 0.0:.3e}, t32 = {t32:.3e}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"


def _ord(t):
    """16-bit floats as integers that count representable values (sign-magnitude -> monotonic)."""
    i = t.detach().cpu().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def _ulps(a, b):
    return int((_ord(a) - _ord(b)).abs().max())


def _status(range_word=True):
    """Wait for the device, then raise what the sync word (and the fp16 range word) hold."""
    import mi355attn
    mi355attn.sync_status(wait=True)
    if range_word:
        mi355attn.range_status(wait=True)


def _run(m, xd):
    """(output, kernel tags) of one forward."""
    import mi355attn
    outs = []
    with torch.no_grad():
        rows = mi355attn.kernel_trace(lambda: outs.append(m(xd)))
    return outs[0], [r[0] for r in rows]
