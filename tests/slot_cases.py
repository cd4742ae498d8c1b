"""Cases of the single-read channel gates' slot-ladder tests (tests/test_slot_cases_cpu.py, tests/test_slot_ladder_gpu.py).

The single-read kernels of SE, ECA, CBAM, SimAM, SRM, GaussianGCT, LCT and GCT keep an image row (CBAM: a band of every channel) in
registers: a lane holds nv = ceil(chunks / 64) 16-byte chunks and the host picks a template instantiation from a bucket ladder over nv
(CBAM: over the segment width, the channel slots per lane and whether the last slot is full).  Every instantiation is its own unrolled
body, so a test only says something about the bodies it runs.  This module

  * restates the host's choice in Python (`choice`: None for the general form, else the kernel, its template arguments and the trace
    tag of the launch), with the place of every restated line; tests/test_slot_cases_cpu.py pins the restatement to the source text
    and the cases to the instantiations of the built library;
  * derives CASES from `choice`, not from a hand-written shape list: per operator and I/O type one shape for every nv with a partly
    filled last slot (64 (nv - 1) + 5 chunks), one exactly full shape per bucket top, the bucket tops again with plain stores
    (option "nt" = 1), the SE variants (weights outside LDS, two workgroups per CU, the biased / hard-sigmoid body) and every
    (SEG, NV, FULL) class of CBAM on one band and on several bands per image;
  * builds three inputs per case, each for one way a slot body goes wrong:
      spread    randn plus an offset in [-2, 2] per (image, channel): a lost or doubled chunk moves a row mean by about
                (offset +- 1) / nv, five orders of magnitude above the bar
      planted   spread with one value of offset + 8 per row, in the row's last live chunk for odd channels and in chunk 0 for even
                channels (CBAM's maxima, SRM's and SimAM's variances then hang on the tail lanes), and a last image that is negative
                throughout (-(0.05 + |randn|) (0.25 + (offset + 2) / 2)), where an idle lane that contributed a 0 to a maximum wins it
      place     a ramp without repeated values inside an image row (fp32: in the whole tensor) under parameters that force a
                constant power-of-two gate (PLACE_GATE): y is that constant times x bit for bit and every element must land in
                its own place

Everything is built on the CPU from fixed seeds; builders are cached, the tests must not modify what they return.
"""
import collections
import functools
import zlib

import torch

import oracle.chan_attn as OC

IOS = ("fp32", "fp16", "bf16")
DTYPE = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
IO_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}                            # the `io` argument of the *16 entries (0: the fp32 entry)
OPS = ("se", "eca", "cbam", "simam", "srm", "gctg", "lct", "gct_l2", "gct_l1")
STAT_MODE = {"simam": 1, "srm": 2, "gctg": 3, "lct": 4, "gct_l2": 5, "gct_l1": 6}      # csrc/chan_stat.h:15
SINGLE_OPTION = {"se": "se_single", "eca": "eca_single", "cbam": "cbam_single"}         # the rest: "zoo_single"
DEFAULTS = dict(nt=3, se_occ=3, io16_occ=4, se_single=1, eca_single=1, cbam_single=1, zoo_single=1)   # csrc/options.h
ECW = 8                                                                 # channel rows per workgroup (csrc/chan_fused.hip:29, chan_stat.h:16)
CUS = 256                                                               # compute units of an MI355X: resident_slots(n) = CUS * n (csrc/api.hip)
B = 3
C_ROWS = 16                                                             # two slices of ECW channels
LCT_GROUPS = 1                                                          # one group of 16 channels: it spans both slices of an image

# ---- the bucket ladders: nv <= entry picks the entry, the last entry takes the rest --------------------------------------------------
LADDERS = {
    ("se", 32): (1, 2, 4, 8, 13, 16),                                   # csrc/chan_fused.hip se_launch_nv
    ("eca", 32): (1, 2, 4, 8, 13, 16),                                  # csrc/chan_fused.hip eca_single, GO ladder
    ("stat", 32): (2, 4, 8, 13, 16),                                    # csrc/chan_stat.hip Stat32::single
    ("se", 16): (1, 2, 4, 7, 8),                                        # csrc/chan_io16.hip:27 se16_nv
    ("eca", 16): (1, 2, 4, 7, 8),                                       # csrc/chan_io16.hip:28 eca16_nv
    ("stat", 16): (1, 2, 4, 7, 8),                                      # csrc/chan_stat_io16.hip:34 stat16_nv
}
MAX_NV = {32: 16, 16: 8}                                                # HW / EPC <= MAX_NV * 64
EPC = {32: 4, 16: 8}                                                    # elements per 16-byte chunk
CBAM_NVS = (4, 8, 16)                                                   # csrc/cbam_band.h:92
CBAM_SEGS = (16, 32)                                                    # csrc/cbam_band.h:88


def bucket(ladder, nv):
    for top in ladder:
        if nv <= top:
            return top
    return ladder[-1]


def se16_waves(nv):                                                     # csrc/chan_io16.hip:33 (nv: a bucket)
    return 8 if nv <= 2 else (6 if nv <= 4 else 4)


def stat16_waves(mode, nv):                                             # csrc/chan_stat_io16.hip:35
    return (6 if nv <= 4 else 4) if mode == 1 else (8 if nv <= 2 else (6 if nv <= 4 else 4))


def stat32_occ(mode, nv):                                               # csrc/chan_stat.hip:245 Stat32::occ
    return (1 if nv > 13 else 2) if mode == 1 else (2 if nv > 13 else 3)


# The lines of host code `choice` restates: (file under csrc/, line, text the line contains).  tests/test_slot_cases_cpu.py reads each
# line back, so a predicate that changes, or moves away from its citation, fails there until `choice` and this table follow.
CITED = (
    ("chan_fused.hip", 290, "if (occ == 3) {"),                        # se_launch: three per CU ignores `nts`
    ("chan_fused.hip", 296, "if (nts && wlds) se_single_kernel<NV, true, true, 2, EXTRA>"),
    ("chan_fused.hip", 320, "return opt(O_ECA_SINGLE) && (HW % 4 == 0) && (HW / 4 <= 16 * 64) && (C % ECW == 0) && (k - 1 <= 8) && (k & 1);"),
    ("chan_fused.hip", 328, "const int nv = (n4 + 63) / 64;"),
    ("chan_fused.hip", 357, "return opt(O_SE_SINGLE) && (HW % 4 == 0) && (HW / 4 <= 16 * 64) && (C % ECW == 0) && ((size_t)(C + Cr) * 4 <= 48 * 1024) &&"),
    ("chan_fused.hip", 358, "C / ECW <= resident_slots(2);"),
    ("chan_fused.hip", 376, "const bool wlds = (size_t)2 * C * Cr * sizeof(float) <= 48 * 1024;"),
    ("chan_fused.hip", 377, "const int nv = (a.n4 + 63) / 64;"),
    ("chan_fused.hip", 380, "const int occ = (opt(O_SE_OCC) == 3 && nv <= 13 && (!wlds || (size_t)(C + Cr + 2 * C * Cr) * 4 <= 50 * 1024)) ? 3 : 2;"),
    ("chan_stat.h", 15, "enum { M_SIMAM = 1, M_SRM = 2, M_GCTG = 3, M_LCT = 4, M_GCT2 = 5, M_GCT1 = 6 };"),
    ("chan_stat.h", 117, "const bool single = mi355::opt(mi355::O_ZOO_SINGLE) && vec && (a.HW / TR::EPC <= TR::MAX_NV * 64) && (C % ECW == 0) &&"),
    ("chan_stat.h", 118, "(size_t)C * 4 <= 48 * 1024 && (MODE != M_LCT || a.i0 <= C) &&"),
    ("chan_stat.h", 119, "(!XCH || C / ECW <= mi355::resident_slots(2));"),
    ("chan_stat.h", 125, "const int nv = (a.nchunk + 63) / 64;"),
    ("chan_stat.hip", 240, "static constexpr int EPC = 4, MAX_NV = 16;"),
    ("chan_stat.hip", 242, "static bool vec(const Args& a) { return (a.HW % 4 == 0) && aligned16(a.x) && aligned16(a.y); }"),
    ("chan_stat.hip", 245, "template <int MODE> static int occ(int nv, size_t) { return MODE == M_SIMAM ? (nv > 13 ? 1 : 2) : (nv > 13 ? 2 : 3); }"),
    ("cbam_band.h", 72, "if (H % R || (R * W) % 4 || R * W > nt / 4) continue;"),
    ("cbam_band.h", 81, "if (!(ks & 1) || ks > 15) return false;"),
    ("cbam_band.h", 88, "g.SEG = g.Q > 16 ? 32 : 16;"),
    ("cbam_band.h", 89, "g.CL = nt / g.SEG;"),
    ("cbam_band.h", 90, "const int nv = (C + g.CL - 1) / g.CL;"),
    ("cbam_band.h", 91, "if (nv > 16) return false;"),
    ("cbam_band.h", 92, "g.NV = nv <= 4 ? 4 : (nv <= 8 ? 8 : 16);"),
    ("cbam_band.h", 96, "const size_t Cp = (size_t)g.CL * g.NV > (size_t)C ? (size_t)g.CL * g.NV : r4(C);"),
    ("cbam_band.h", 97, "g.smem_base = (3 * Cp + 2 * r4(Cr) + 2 * r4((size_t)g.NB * g.cpb) + 2 * (size_t)g.CL * g.SEG * 4 +"),
    ("cbam_band.h", 98, "r4(2 * (size_t)TH * TW) + (size_t)g.SEG * 4 + r4(2 * (size_t)ks * ks)) * 4;"),
    ("cbam_band.h", 100, "if (full16 && g.NV == 16 && C != g.CL * g.NV) return false;"),
    ("cbam_band.h", 101, "return g.smem_base <= 40 * 1024;"),
    ("cbam_single.hip", 321, "return geometry(512, C, Cr, H, W, ks, false, g);"),
    ("cbam_single.hip", 340, "return opt(O_CBAM_SINGLE) && pick_geometry(C, Cr, H, W, ks, g) && g.NB <= resident_slots(2);"),
    ("cbam_single.hip", 361, "const bool full = (C == g.CL * g.NV);"),
    ("chan_io16.hip", 27, "constexpr int se16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }"),
    ("chan_io16.hip", 28, "constexpr int eca16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }"),
    ("chan_io16.hip", 33, "constexpr int se16_waves(int nv) { return nv <= 2 ? 8 : (nv <= 4 ? 6 : 4); }"),
    ("chan_io16.hip", 689, "return mi355::opt(mi355::O_ECA_SINGLE) && (HW % 8 == 0) && (HW / 8 <= 8 * 64) && (C % ECW == 0) && (k - 1 <= 8) && (k & 1);"),
    ("chan_io16.hip", 721, "return mi355::opt(mi355::O_SE_SINGLE) && (HW % 8 == 0) && (HW / 8 <= 8 * 64) && (C % ECW == 0) && ((size_t)(C + Cr) * 4 <= 48 * 1024) &&"),
    ("chan_io16.hip", 722, "C / ECW <= mi355::resident_slots(2);"),
    ("chan_io16.hip", 741, "const bool wlds = (size_t)(C + Cr + 2 * (size_t)C * Cr) * sizeof(float) <= 60 * 1024;"),
    ("chan_io16.hip", 743, "const int nv = (a.HW / 8 + 63) / 64;"),
    ("chan_io16.hip", 745, "if (occ > se16_waves(se16_nv(nv)) / 2) occ = se16_waves(se16_nv(nv)) / 2;"),
    ("chan_io16.hip", 746, "while (occ > 2 && smem * occ > 150 * 1024) --occ;"),
    ("chan_io16.hip", 771, "return mi355::opt(mi355::O_CBAM_SINGLE) && geometry(512, C, Cr, H, W, ks, true, g) && g.NB <= mi355::resident_slots(2) &&"),
    ("chan_io16.hip", 793, "const bool full = (C == g.CL * g.NV);"),
    ("chan_stat_io16.hip", 34, "constexpr int stat16_nv(int nv) { return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : (nv <= 7 ? 7 : 8))); }"),
    ("chan_stat_io16.hip", 35, "constexpr int stat16_waves(int mode, int nv) { return mode == M_SIMAM ? (nv <= 4 ? 6 : 4) : (nv <= 2 ? 8 : (nv <= 4 ? 6 : 4)); }"),
    ("chan_stat_io16.hip", 337, "static constexpr int EPC = 8, MAX_NV = 8;"),
    ("chan_stat_io16.hip", 339, "static bool vec(const Args& a) { return (a.HW % 8 == 0) && aligned16(a.x) && aligned16(a.y); }"),
    ("chan_stat_io16.hip", 343, "int n = stat16_waves(MODE, stat16_nv(nv)) / 2;"),
    ("chan_stat_io16.hip", 344, "while (n > 2 && (smem + 256) * n > 150 * 1024) --n;"),
)


# ---- CBAM band geometry (csrc/cbam_band.h) ---------------------------------------------------------------------------------------------
def band_rows(H, W, nt=512):
    """cbam_band.h:69-76: the most rows per band with R | H, (R * W) % 4 == 0 and R * W <= nt / 4; 0 if none."""
    best = 0
    for R in range(1, H + 1):
        if H % R or (R * W) % 4 or R * W > nt // 4:
            continue
        best = R
    return best


Geo = collections.namedtuple("Geo", "R Q NB SEG CL NV cpb smem_base smem_w")


def geometry(C, Cr, H, W, ks, full16, nt=512):
    """cbam_band.h:80-102; None where the source returns false."""
    if not (ks & 1) or ks > 15:
        return None
    R = band_rows(H, W, nt)
    if not R:
        return None
    Q, NB = R * W // 4, H // R
    SEG = 32 if Q > 16 else 16
    CL = nt // SEG
    nv = (C + CL - 1) // CL
    if nv > 16:
        return None
    NV = 4 if nv <= 4 else (8 if nv <= 8 else 16)
    cpb = (C + NB - 1) // NB
    pad = (ks - 1) // 2
    TW, TH = W + 2 * pad, R + 2 * pad
    r4 = lambda n: (n + 3) & ~3
    Cp = CL * NV if CL * NV > C else r4(C)
    smem_base = (3 * Cp + 2 * r4(Cr) + 2 * r4(NB * cpb) + 2 * CL * SEG * 4 + r4(2 * TH * TW) + SEG * 4 + r4(2 * ks * ks)) * 4
    if full16 and NV == 16 and C != CL * NV:
        return None
    if smem_base > 40 * 1024:
        return None
    return Geo(R, Q, NB, SEG, CL, NV, cpb, smem_base, 2 * C * Cr * 4)


# ---- the host's choice -------------------------------------------------------------------------------------------------------------------
Choice = collections.namedtuple("Choice", "kernel targs tag nv NV wg_per_cu")   # targs: as the demangled symbol lists them


def inst(c):
    return (c.kernel, c.targs)


def choice(op, io, C, Cr, H, W, ks=0, options=None, extra=False, cus=CUS):
    """What the host launches for a dense, 16-byte aligned (B, C, H, W) tensor of I/O type `io`: None for the general form, else a Choice.
    Cr: hidden width (SE, CBAM); ks: ECA's taps / CBAM's kernel size; extra: SE with biases or the hard-sigmoid gate; options: values
    that differ from DEFAULTS; cus: compute units of the device.  nv: chunks per lane (0: CBAM), NV: the slot count of the instantiation,
    wg_per_cu: workgroups per CU the grid is sized for (0: ECA, one workgroup per slice)."""
    o = dict(DEFAULTS, **(options or {}))
    bits = 32 if io == "fp32" else 16
    code = IO_CODE[io]
    HW = H * W
    nts = bool(o["nt"] & 2)
    epc, top = EPC[bits], MAX_NV[bits]
    rows_fit = HW % epc == 0 and HW // epc <= top * 64 and C % ECW == 0
    nv = (HW // epc + 63) // 64
    if op == "se":
        # chan_fused.hip:353-358 se_single_applicable; chan_io16.hip:717-723 se16_single_ok (vec: chan_attn.hip:458, chan_io16.hip:871)
        if not (o["se_single"] and rows_fit and (C + Cr) * 4 <= 48 * 1024 and C // ECW <= 2 * cus):
            return None
        if bits == 32:
            wlds = 2 * C * Cr * 4 <= 48 * 1024                                             # chan_fused.hip:376
            occ = 3 if (o["se_occ"] == 3 and nv <= 13 and (not wlds or (C + Cr + 2 * C * Cr) * 4 <= 50 * 1024)) else 2   # :380
            NV = bucket(LADDERS["se", 32], nv)
            nts_t = occ == 3 or nts                                                        # se_launch: three per CU is built with NT stores only
            tag = f"se_single_kernel C={C} HW={HW} nv={nv} NV={NV} occ={occ} wlds={int(wlds)} extra={int(extra)} nts={int(nts_t)}"
            return Choice("se_single_kernel", (NV, nts_t, wlds, occ, bool(extra)), tag, nv, NV, occ)
        wlds = (C + Cr + 2 * C * Cr) * 4 <= 60 * 1024                                      # chan_io16.hip:741
        NV = bucket(LADDERS["se", 16], nv)
        smem = (C + Cr + (2 * C * Cr if wlds else 0)) * 4
        occ = min(o["io16_occ"], se16_waves(NV) // 2)                                      # chan_io16.hip:744-746
        while occ > 2 and smem * occ > 150 * 1024:
            occ -= 1
        tag = f"se16_single_kernel io={code} C={C} HW={HW} nv={nv} NV={NV} wlds={int(wlds)} extra={int(extra)}"
        return Choice("se16_single_kernel", (code, NV, wlds, bool(extra)), tag, nv, NV, occ)
    if op == "eca":
        # chan_fused.hip:318-321 eca_single_applicable; chan_io16.hip:687-690 eca16_single_ok.  One workgroup per slice: no residency.
        if not (o["eca_single"] and rows_fit and ks - 1 <= 8 and ks & 1):
            return None
        NV = bucket(LADDERS["eca", bits], nv)
        if bits == 32:
            tag = f"eca_halo_kernel C={C} HW={HW} k={ks} nv={nv} NV={NV} nts={int(nts)}"
            return Choice("eca_halo_kernel", (NV, nts), tag, nv, NV, 0)
        tag = f"eca16_halo_kernel io={code} C={C} HW={HW} k={ks} nv={nv} NV={NV}"
        return Choice("eca16_halo_kernel", (code, NV), tag, nv, NV, 0)
    if op == "cbam":
        # cbam_single.hip:337-341 cbam_single_applicable; chan_io16.hip:768-773 cbam16_single_ok
        g = geometry(C, Cr, H, W, ks, full16=bits == 16)
        if not (o["cbam_single"] and g is not None and g.NB <= 2 * cus):
            return None
        full = C == g.CL * g.NV                                                            # cbam_single.hip:361, chan_io16.hip:793
        if bits == 32:
            tag = f"cbam_single_kernel C={C} H={H} W={W} ks={ks} SEG={g.SEG} NV={g.NV} full={int(full)}"
            return Choice("cbam_single_kernel", (512, g.SEG, g.NV, full), tag, 0, g.NV, 2)
        tag = f"cbam16_single_kernel io={code} C={C} H={H} W={W} ks={ks} SEG={g.SEG} NV={g.NV} full={int(full)}"
        return Choice("cbam16_single_kernel", (code, g.SEG, g.NV, full), tag, 0, g.NV, 2)
    mode = STAT_MODE[op]
    xch = mode >= 3
    # chan_stat.h:117-119 stat_run's `single` (LCT's a.i0 <= C always holds: i0 = C / groups)
    if not (o["zoo_single"] and rows_fit and C * 4 <= 48 * 1024 and (not xch or C // ECW <= 2 * cus)):
        return None
    if op in ("simam", "srm") and HW < 2:
        return None                                                                        # the entries refuse one pixel
    NV = bucket(LADDERS["stat", bits], nv)
    if bits == 32:
        tag = f"stat_single_kernel mode={mode} C={C} HW={HW} nv={nv} NV={NV} nts={int(nts)}"
        return Choice("stat_single_kernel", (mode, NV, nts), tag, nv, NV, stat32_occ(mode, nv))
    occ = stat16_waves(mode, NV) // 2                                                      # chan_stat_io16.hip:342-346 Stat16::occ
    smem = C * 4 if xch else 0
    while occ > 2 and (smem + 256) * occ > 150 * 1024:
        occ -= 1
    tag = f"stat16_single_kernel io={code} mode={mode} C={C} HW={HW} nv={nv} NV={NV}"
    return Choice("stat16_single_kernel", (code, mode, NV), tag, nv, NV, occ)


_TAG_FIELDS = {                                                         # kernel -> the tag's keys that are its template arguments, in order
    "se_single_kernel": ("NV", "nts", "wlds", "occ", "extra"), "eca_halo_kernel": ("NV", "nts"), "stat_single_kernel": ("mode", "NV", "nts"),
    "cbam_single_kernel": ("SEG", "NV", "full"), "se16_single_kernel": ("io", "NV", "wlds", "extra"), "eca16_halo_kernel": ("io", "NV"),
    "stat16_single_kernel": ("io", "mode", "NV"), "cbam16_single_kernel": ("io", "SEG", "NV", "full"),
}
_BOOLS = ("nts", "wlds", "extra", "full")
KERNELS = tuple(_TAG_FIELDS)


def inst_of_tag(tag):
    """(kernel, template arguments) named by a trace tag of one of the eight single-read launches; None for any other tag."""
    name, _, rest = tag.partition(" ")
    if name not in _TAG_FIELDS:
        return None
    kv = dict(f.split("=") for f in rest.split())
    targs = tuple(bool(int(kv[k])) if k in _BOOLS else int(kv[k]) for k in _TAG_FIELDS[name])
    return (name, (512,) + targs if name == "cbam_single_kernel" else targs)


def targs_text(targs):
    """Template arguments as a demangled symbol prints them."""
    return ", ".join(("true" if v else "false") if isinstance(v, bool) else str(v) for v in targs)


# Compiled instantiations no shape or option reaches, with the line of host code that excludes each: (kernel, targs) -> reason.
# Empty: the launch tables instantiate exactly what they can pick (se_launch builds no plain-store kernel for three workgroups per CU,
# cbam16_single names <IO, SEG, 16, true> alone), and the CPU test fails as soon as a compiled body is neither here nor reached.
UNREACHABLE = {}


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "id op io B C Cr H W ks opts extra kind")):
    """opts: sorted ((option, value), ...) the case runs under; extra: None, "bias" (SELayerBias) or "hsig" (SqueezeExcite)."""
    __slots__ = ()

    @property
    def options(self):
        return dict(self.opts)

    @property
    def shape(self):
        return (self.B, self.C, self.H, self.W)

    @property
    def dtype(self):
        return DTYPE[self.io]

    def choice(self, cus=CUS, **more):
        return choice(self.op, self.io, self.C, self.Cr, self.H, self.W, self.ks, dict(self.options, **more), bool(self.extra), cus)


def eca_taps(C):
    return OC.eca_kernel_size(C)


def _mk(op, io, H, W, kind, C=C_ROWS, Cr=None, ks=0, opts=None, extra=None, batch=B):
    if Cr is None:
        Cr = (C // 16 if C >= 32 else C // 4) if op in ("se", "cbam") else 0
    if op == "eca":
        ks = eca_taps(C)
    opts = tuple(sorted((opts or {}).items()))
    cid = f"{op}-{io}-{kind}-C{C}r{Cr}-{H}x{W}" + (f"-k{ks}" if op == "cbam" else "") + (f"-{extra}" if extra else "") + \
        "".join(f"-{k}{v}" for k, v in opts)
    return Case(cid, op, io, batch, C, Cr, H, W, ks, opts, extra, kind)


def ragged_shape(io, nv):
    """A map of 64 (nv - 1) + 5 chunks: the last slot holds five live lanes."""
    chunks = 64 * (nv - 1) + 5
    return (4, chunks) if io == "fp32" else (8, chunks)


def full_shape(io, nv):
    """A map of exactly 64 nv chunks."""
    return (16, 16 * nv) if io == "fp32" else (16, 32 * nv)


def _row_cases(op, io):
    bits = 32 if io == "fp32" else 16
    fam = op if op in ("se", "eca") else "stat"
    ladder = LADDERS[fam, bits]
    out = []
    for nv in range(1, MAX_NV[bits] + 1):
        out.append((_mk(op, io, *ragged_shape(io, nv), kind=f"ragged{nv}"), nv))
    for top in ladder:
        out.append((_mk(op, io, *full_shape(io, top), kind=f"full{top}"), top))
        out.append((_mk(op, io, *full_shape(io, top), kind=f"full{top}", opts=dict(nt=1)), top))
    if op == "se":
        out += _se_variants(io, ladder)
    cases = []
    for c, nv in out:
        ch = c.choice()
        assert ch is not None and ch.nv == nv and ch.NV == bucket(ladder, nv), (c, ch)
        cases.append(c)
    return cases


def smallest_unstaged_c(io):
    """The smallest SELayer(C) (reduction 16) whose weight matrices the single-read kernel leaves in global memory."""
    for C in range(32, 4096, ECW):
        ch = choice("se", io, C, C // 16, 16, 16)
        if ch is not None and not ch.targs[2]:
            return C
    raise AssertionError("no channel count leaves the SE weights outside LDS")


def _se_variants(io, ladder):
    """Every other instantiation of the SE kernels at the bucket tops: weights in LDS or not, the body with biases / hard sigmoid, and
    (fp32) two workgroups per CU with non-temporal and with plain stores; the LDS corner that forces two per CU on its own."""
    out = []
    wide = smallest_unstaged_c(io)
    variants = [{}, dict(se_occ=2), dict(se_occ=2, nt=1)] if io == "fp32" else [{}]
    for C in (C_ROWS, wide):
        for extra in (None, "hsig" if C == C_ROWS else "bias"):
            for opts in variants:
                if C == C_ROWS and extra is None and not opts:
                    continue                                            # the plain sweep
                for top in ladder:
                    out.append((_mk("se", io, *full_shape(io, top), kind=f"full{top}", C=C, opts=opts, extra=extra), top))
    if io == "fp32":
        # SELayer(768, 96): W1 and W2 fill 48 KiB of LDS exactly, with p and h beside them more than three workgroups' share
        c = _mk("se", io, *ragged_shape(io, 2), kind="ldscorner2", C=768, Cr=8)
        assert c.choice().targs == (2, True, True, 2, False), c.choice()
        out.append((c, 2))
    return out


@functools.lru_cache(maxsize=None)
def cbam_maps():
    """{(SEG, several bands?): (H, W)}: the smallest maps whose bands hold 12 (SEG 16) or 20 (SEG 32) pixel quads -- the segment's last
    lanes idle -- as one band per image and as several."""
    found = {}
    for H in range(1, 17):
        for W in range(4, 68, 4):
            g = geometry(64, 4, H, W, 7, False)
            if g is None or g.Q not in (12, 20):
                continue
            key = (g.SEG, g.NB > 1)
            rank = lambda hw: (hw[0] * hw[1], abs(hw[0] - hw[1]))     # fewest pixels, then the squarest
            if key not in found or rank((H, W)) < rank(found[key]):
                found[key] = (H, W)
    assert set(found) == {(s, m) for s in CBAM_SEGS for m in (False, True)}, found
    return found


def _cbam_cases(io):
    cases = []
    maps = cbam_maps()
    for SEG in CBAM_SEGS:
        CL = 512 // SEG
        for NV in CBAM_NVS:
            for full in (True, False):
                C = CL * NV - (0 if full else 3)
                for several in (False, True):
                    c = _mk("cbam", io, *maps[SEG, several], kind=f"seg{SEG}nv{NV}{'full' if full else 'part'}{'-bands' if several else ''}",
                            C=C, ks=7)
                    ch = c.choice()
                    if io != "fp32" and NV == 16 and not full:
                        assert ch is None, c                            # cbam_band.h:100: the 16-bit kernel leaves these to the general form
                        continue
                    assert ch is not None and ch.targs[-3:] == (SEG, NV, full), (c, ch)
                    cases.append(c)
        c = _mk("cbam", io, *maps[SEG, False], kind=f"seg{SEG}nv4full", C=CL * 4, ks=3)
        assert c.choice().targs[-3:] == (SEG, 4, True)
        cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def cases(op, io):
    out = _cbam_cases(io) if op == "cbam" else _row_cases(op, io)
    assert len({c.id for c in out}) == len(out), [c.id for c in out]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(c for op in OPS for io in IOS for c in cases(op, io))


def reachable(op=None, io=None, cus=CUS):
    """The instantiations the cases reach, by the host's choice."""
    return {inst(c.choice(cus)) for c in all_cases() if (op is None or c.op == op) and (io is None or c.io == io)}


def many_slices_case(op, io, cus=CUS):
    """Bucket 8 with more slices than resident workgroups: (the plain ragged case at nv = 7 (fp32) / 6 (16-bit), the image count
    3 * cus / (C / 8) + 1 at which a workgroup walks several slices).  The images of the long batch are the case's three, repeated."""
    nv = 7 if io == "fp32" else 6
    base = next(c for c in cases(op, io) if c.kind == f"ragged{nv}" and not c.opts and not c.extra and c.C == C_ROWS)
    return base, 3 * cus // (base.C // ECW) + 1


# ---- parameters and the oracle -----------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def params(op, C, Cr, ks, extra):
    """fp32 CPU parameters of the case's module, O(1) and non-trivial (the defaults make GCT and SRM's BatchNorm the identity)."""
    g = _gen("params", op, C, Cr, ks, extra)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    if op in ("se", "cbam"):
        p = dict(w1=0.5 * rn(Cr, C) / C ** 0.5, w2=rn(C, Cr) / Cr ** 0.5)
        if op == "cbam":
            p["wconv"] = rn(1, 2, ks, ks) * (0.5 / ks)
        if extra:
            p["b1"], p["b2"] = 0.5 * rn(Cr), (1.5 if extra == "hsig" else 0.5) * rn(C)
        return p
    if op == "eca":
        return dict(taps=0.5 * rn(1, 1, ks))
    if op == "srm":
        return dict(cfc=rn(C, 1, 2), bn_w=0.5 + ru(C), bn_b=0.5 * rn(C), bn_mean=0.3 * rn(C), bn_var=0.5 + ru(C))
    if op == "lct":
        return dict(w=rn(C), b=rn(C))
    if op in ("gct_l2", "gct_l1"):
        return dict(alpha=0.5 + ru(1, C, 1, 1), gamma=rn(1, C, 1, 1), beta=0.5 * rn(1, C, 1, 1))
    return {}


def case_params(c):
    return params(c.op, c.C, c.Cr, c.ks, c.extra)


PLACE_OPS = ("se", "eca", "cbam", "gct_l2")
PLACE_GATE = {"se": 0.5, "eca": 0.5, "cbam": 0.25, "gct_l2": 1.0}      # sigmoid(0); sigmoid(0) sigmoid(0); 1 + tanh(0)


def place_params(c):
    """The case's parameters with what forces the constant gate: SE and CBAM w2 = 0 (CBAM: zero conv weights too), ECA zero taps, GCT
    gamma = beta = 0."""
    p = {k: v.clone() for k, v in case_params(c).items()}
    for k in {"se": ("w2", "b2"), "eca": ("taps",), "cbam": ("w2", "wconv"), "gct_l2": ("gamma", "beta")}[c.op]:
        if k in p:
            p[k].zero_()
    return p


def oracle(c, x, p, dtype=torch.float64):
    """The reference of case c's module on x (fp32, or the 16-bit tensor itself: widened exactly) with parameters p, computed in `dtype`."""
    x = x.to(dtype)
    if c.op == "se":
        if c.extra:
            return OC.se_ex_forward(x, p["w1"], p["b1"], p["w2"], p["b2"], "hard_sigmoid" if c.extra == "hsig" else "sigmoid", dtype=dtype)
        return OC.se_forward(x, p["w1"], p["w2"], dtype=dtype)
    if c.op == "eca":
        return OC.eca_forward(x, p["taps"], dtype=dtype)
    if c.op == "cbam":
        return OC.cbam_forward(x, p["w1"], p["w2"], p["wconv"], dtype=dtype)
    if c.op == "simam":
        return OC.simam_forward(x, 1e-4, dtype=dtype)
    if c.op == "srm":
        return OC.srm_forward(x, p["cfc"], p["bn_w"], p["bn_b"], p["bn_mean"], p["bn_var"], 1e-5, dtype=dtype)
    if c.op == "gctg":
        return OC.gct_gauss_forward(x, 2, 1e-5, dtype=dtype)
    if c.op == "lct":
        return OC.lct_forward(x, p["w"], p["b"], LCT_GROUPS, 1e-5, dtype=dtype)
    return OC.gct_forward(x, p["alpha"], p["gamma"], p["beta"], 1e-5, "l2" if c.op == "gct_l2" else "l1", False, dtype=dtype)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
PLANT = 8.0
TOL32 = {op: (1e-5 if op in ("se", "eca", "cbam") else 2e-5) for op in OPS}     # assert_parity bars of tests/test_chan_attn_gpu.py
TOL32_GENERAL = {op: (1e-6 if op in ("se", "eca") else 2e-6) for op in OPS}     # single read against the general form, same file
T32_IO16 = 1e-5                                                                 # the fp32 term of io16_common._check_chan


def planted_at(c):
    """(index inside a row for even channels, for odd channels): an element of chunk 0 and one of the row's last live chunk."""
    return 1, c.H * c.W - 2


@functools.lru_cache(maxsize=8)
def make_input(c, kind):
    """x of case c in its I/O type (CPU): "spread", "planted" or "place" (module docstring)."""
    Bn, C, H, W = c.shape
    HW = H * W
    if kind == "place":
        return _ramp(c)
    g = _gen("x", c.shape, c.io)
    off = 4.0 * torch.rand(Bn, C, 1, generator=g) - 2.0
    x = torch.randn(Bn, C, HW, generator=g)
    if kind == "planted":
        neg = -(0.05 + x[-1].abs()) * (0.25 + 0.5 * (off[-1] + 2.0))    # scaled per row: GCT / LCT divide by the spread of the row means
        x = x + off
        lo, hi = planted_at(c)
        x[:, 0::2, lo] = off[:, 0::2, 0] + PLANT
        x[:, 1::2, hi] = off[:, 1::2, 0] + PLANT
        x[-1] = neg
    else:
        assert kind == "spread", kind
        x = x + off
    return x.reshape(c.shape).to(c.dtype)


def _ramp(c):
    Bn, C, H, W = c.shape
    HW, rows = H * W, Bn * C
    if c.io == "fp32":
        n = rows * HW
        assert n < 1 << 24
        x = (torch.arange(1, n + 1, dtype=torch.float32) * 2.0 ** -12).reshape(rows, HW)
        x[1::2] = -x[1::2]
        return x.reshape(c.shape)
    # positive normal bit patterns, far enough from both ends that a quarter of each value is exact: fp16 2^-7 .. 2^13, bf16 2^-31 .. 2^33
    lo, hi = (0x2000, 0x7000) if c.io == "fp16" else (0x3000, 0x5000)
    assert HW <= hi - lo
    start = (torch.arange(rows, dtype=torch.int64) * 977) % (hi - lo - HW + 1)
    bits = lo + start[:, None] + torch.arange(HW, dtype=torch.int64)[None, :]
    bits[1::2] += 0x8000                                                # odd rows negative
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(c.dtype).reshape(c.shape)
