"""CPU guard for the fp16 range contract (include/mi355attn.h, fp16 range guard): every HIP source that converts a value to a 16-bit MFMA
operand either reports saturations into the range word (an rg_report call) or is named below with the reason it needs none.  A new
kernel that converts without reporting fails here, before it reaches a GPU."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch-attention_amd", "csrc")

# fp32 -> 16-bit conversions: the operand traits of mma.h (M_::cvt / cvt1, Mma<P>::cvt), C-style and static casts to the 16-bit types,
# and a kernel launched with an fp16 template argument (the templated converters: T(x) / (T)x inside).
CONVERSION = re.compile(r"M_::cvt|Mma<[^>]*>::cvt|\((?:_Float16|__bf16)\)|static_cast<(?:_Float16|__bf16)>|_kernel<[^>]*_Float16[^>]*><<<")

ALLOW = {
    "mma.h": "the operand traits themselves",
    "yardstick.hip": "measurement kernel, not reachable from a module",
    "ln_fold.hip": "converts LayerNorm-centred rows; its entry hands the range word to the folding GEMM epilogue, which reports (code 5)",
    "xcit.hip": "KNOWN GAP: xca_kernel<D, _Float16> on an fp32 qkv (mi355_xca16_fwd, qkv_is16 = 0) does not report its v staging",
}


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_every_converting_source_reports_or_is_allow_listed():
    missing = []
    for path in _sources():
        name = os.path.basename(path)
        src = open(path).read()
        if CONVERSION.search(src) and "rg_report" not in src and name not in ALLOW:
            missing.append(name)
    assert not missing, f"fp32 -> 16-bit conversions without a range report (add rg_report + range_word(), or allow-list with a reason): {missing}"


def test_allow_list_is_current():
    """An allow-listed file that no longer converts, or now reports, leaves the list (so the list never hides a new kernel)."""
    names = {os.path.basename(p): open(p).read() for p in _sources()}
    stale = [n for n in ALLOW if n not in names or not CONVERSION.search(names[n]) or ("rg_report" in names[n] and n != "mma.h")]
    assert not stale, stale


def test_detector_sees_the_known_forms():
    for line in ("const v4 h = M_::cvt(v);", "o[k] = (_Float16)s[k];", "w16[i] = (__bf16)wA[i];",
                 "if (p) im2col16_kernel<_Float16><<<blocks, 256, shm, st>>>(img);"):
        assert CONVERSION.search(line), line
    assert not CONVERSION.search("const float f = (float)h;")
