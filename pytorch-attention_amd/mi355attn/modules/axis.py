"""Drop-in modules for four more members of the reference's attention zoo whose gates come from AXIS reductions of
the NCHW activation (csrc/axis_attn.hip):

  GCModule             attention_mechanisms/gc_module.py:17-43          global context (no softmax, as in the reference) -> bottleneck
                                                                        transform with LayerNorm -> added to every position
  CoordinateAttention  attention_mechanisms/coordatten.py:18-44         row / column means -> shared 1x1 conv + BN + ReLU -> two 1x1 convs
  TripletAttention     attention_mechanisms/triplet_attention.py:19-63  three rotated AttentionGates, averaged
  BAM                  attention_mechanisms/bam.py:16-71                channel gate (MLP + BN1d) + spatial gate (dilated convs) -> sigmoid

Same constructor signatures, submodule names and state_dict keys as the reference.  BatchNorm layers run in eval mode (running
statistics); calling forward() in training mode raises.  The helper classes that only exist as parameter containers in the
reference (BasicConv2d, ZPool, AttentionGate, ChannelGate, SpatialGate) keep their names and parameters; the fused forward lives in
the top-level module.

CoordinateAttention, TripletAttention, AttentionGate and BAM also take an fp16 / bf16 device tensor and return the same type
(csrc/axis_attn_io16.hip: 16-bit sweeps over x and y, fp32 gates in between); their parameters may then be 16-bit too.  GCModule and the
parameter-container helpers (ZPool, BasicConv2d, ChannelGate, SpatialGate) are fp32 only.
"""
import torch
from torch import nn

from .. import functional as F


def _eval_only(m):
    if m.training:
        raise RuntimeError("inference engine: BatchNorm runs with its running statistics; call .eval()")


class GCModule(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.conv = nn.Conv2d(channel, 1, kernel_size=1)
        self.softmax = nn.Softmax(dim=2)            # declared and unused in the reference (gc_module.py:22, :30-38)
        self.transform = nn.Sequential(
            nn.Conv2d(channel, channel // reduction, kernel_size=1),
            nn.LayerNorm([channel // reduction, 1, 1]),
            nn.ReLU(inplace=True),
            nn.Conv2d(channel // reduction, channel, kernel_size=1),
        )

    def forward(self, x):
        t = self.transform
        return F.gc_forward(x, self.conv.weight, self.conv.bias, t[0].weight, t[0].bias, t[1].weight, t[1].bias, t[1].eps,
                            t[3].weight, t[3].bias)


class CoordinateAttention(nn.Module):
    def __init__(self, in_dim, out_dim, reduction=32):
        super().__init__()
        self.pool_h = nn.AdaptiveAvgPool2d((None, 1))
        self.pool_w = nn.AdaptiveAvgPool2d((1, None))
        hidden_dim = max(8, in_dim // reduction)
        self.conv1 = nn.Conv2d(in_dim, hidden_dim, kernel_size=1, stride=1, padding=0)
        self.bn1 = nn.BatchNorm2d(hidden_dim)
        self.act = nn.ReLU(inplace=True)
        self.conv_h = nn.Conv2d(hidden_dim, out_dim, kernel_size=1, stride=1, padding=0)
        self.conv_w = nn.Conv2d(hidden_dim, out_dim, kernel_size=1, stride=1, padding=0)
        self.in_dim, self.out_dim = in_dim, out_dim

    def forward(self, x):
        _eval_only(self)
        if self.out_dim != self.in_dim:
            raise ValueError("CoordinateAttention: identity * a_h * a_w (coordatten.py:43) needs out_dim == in_dim")
        scale, shift = F.bn_fold(self.bn1)
        return F.coordatt_forward(x, self.conv1.weight, self.conv1.bias, scale, shift, self.conv_h.weight, self.conv_h.bias,
                                  self.conv_w.weight, self.conv_w.bias)


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, ks):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=ks, stride=1, padding=(ks - 1) // 2)
        self.bn = nn.BatchNorm2d(out_channels)
        self.act = nn.ReLU(inplace=True)

    def forward(self, x):
        """conv -> bn -> relu (triplet_attention.py:25-29) on its own: the implicit-GEMM conv with the BatchNorm folded into its rows
        and a ReLU epilogue, then the token rows back to NCHW.  (Inside TripletAttention the 2 -> 1 gates run fused instead.)"""
        _eval_only(self)
        ks = self.conv.kernel_size[0]
        s, t = F.bn_fold(self.bn, self.conv.bias)
        tag = (id(s), self.conv.weight._version, self.conv.weight.data_ptr())
        rows = F._derived_get((self.conv.weight, self.bn), ("basicconv_rows",), tag,
                              lambda: F._gemm_rows(self.conv.weight.detach() * s[:, None, None, None], 0))
        B, _, H, W = x.shape
        tok, (oh, ow) = F.conv2d_tokens(x, None, t, ks, 1, (ks - 1) // 2, 0, precision=F.PREC_STRICT, act=F.ACT_RELU, wrows=rows)
        return F.tokens_to_nchw(tok, oh, ow)


class ZPool(nn.Module):
    def forward(self, x):
        return F.zpool(x)                                     # triplet_attention.py:31-36


class AttentionGate(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.compress = ZPool()
        self.conv = BasicConv2d(2, 1, kernel_size)
        self.activation = nn.Sigmoid()

    def forward(self, x):
        """x * sigmoid(conv(compress(x))) (triplet_attention.py:45-49) on its own, through the same gate kernel TripletAttention uses."""
        _eval_only(self)
        s, t = F.bn_fold(self.conv.bn, self.conv.conv.bias)
        tag = (id(s), id(t))
        affine = F._derived_get((self.conv.bn,), ("gate_affine",), tag, lambda: torch.cat([s, t]).contiguous())
        return F.attention_gate(x, self.conv.conv.weight, affine, self.conv.conv.kernel_size[0])


class TripletAttention(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.ch = AttentionGate(kernel_size)
        self.cw = AttentionGate(kernel_size)
        self.hw = AttentionGate(kernel_size)
        self.kernel_size = kernel_size

    def _affine(self):
        gates = (self.ch, self.cw, self.hw)
        folds = [F.bn_fold(g.conv.bn, g.conv.conv.bias) for g in gates]
        tag = tuple(id(t) for f in folds for t in f)

        def build():
            return torch.cat([torch.cat([s, t]) for s, t in folds]).contiguous()

        return F._derived_get((self,), ("triplet_affine",), tag, build), folds

    def forward(self, x):
        _eval_only(self)
        affine, _keep = self._affine()
        return F.triplet_forward(x, self.ch.conv.conv.weight, self.cw.conv.conv.weight, self.hw.conv.conv.weight, affine,
                                 self.kernel_size)


class ChannelGate(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.mlp = nn.Sequential(
            nn.Linear(channel, channel // reduction),
            nn.ReLU(inplace=True),
            nn.Linear(channel // reduction, channel),
        )
        self.bn = nn.BatchNorm1d(channel)

    def forward(self, x):
        """bn(mlp(avgpool(x))) expanded over the image (bam.py:28-33), computed by the kernels of the fused BAM forward."""
        _eval_only(self)
        Cr = self.mlp[0].weight.shape[0]
        bn1d = F.bn_fold(self.bn)
        dummy = x.new_zeros(1)
        params = [self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight, self.mlp[2].bias, bn1d[0], bn1d[1]] + [dummy] * 10
        cg, _ = F.bam_gates(x, params, Cr, 1, channel=True, spatial=False)
        return cg.view(x.shape[0], x.shape[1], 1, 1).expand_as(x)


class SpatialGate(nn.Module):
    def __init__(self, channel, reduction=16, kernel_size=3, dilation_val=4):
        super().__init__()
        self.conv1 = nn.Conv2d(channel, channel // reduction, kernel_size=1)
        self.conv2 = nn.Sequential(
            nn.Conv2d(channel // reduction, channel // reduction, kernel_size, padding=dilation_val, dilation=dilation_val),
            nn.BatchNorm2d(channel // reduction),
            nn.ReLU(inplace=True),
            nn.Conv2d(channel // reduction, channel // reduction, kernel_size, padding=dilation_val, dilation=dilation_val),
            nn.BatchNorm2d(channel // reduction),
            nn.ReLU(inplace=True),
        )
        self.conv3 = nn.Conv2d(channel // reduction, 1, kernel_size=1)
        self.bn = nn.BatchNorm2d(1)
        self.kernel_size, self.dilation = kernel_size, dilation_val

    def _folded(self):
        """Parameters 6..15 of the BAM table: conv1, the two dilated convs with their BatchNorms folded, conv3 with bn folded."""
        if self.kernel_size != 3:
            raise ValueError("SpatialGate: the kernel is written for 3x3 dilated convolutions (bam.py:36)")
        d1 = F.bn_fold(self.conv2[1], self.conv2[0].bias)
        d2 = F.bn_fold(self.conv2[4], self.conv2[3].bias)
        s, t = F.bn_fold(self.bn, self.conv3.bias)
        tag = (id(s), self.conv3.weight._version, self.conv3.weight.data_ptr())
        w3, b3 = F._derived_get((self.conv3.weight, self.bn), ("bam_conv3",), tag,
                                lambda: ((self.conv3.weight.detach().float().reshape(-1) * s).contiguous(), t))   # fp32, as bn_fold
        return [self.conv1.weight, self.conv1.bias, self.conv2[0].weight, d1[0], d1[1], self.conv2[3].weight, d2[0], d2[1], w3, b3]

    def forward(self, x):
        """bn(conv3(conv2(conv1(x)))) expanded over the channels (bam.py:53-59), computed by the kernels of the fused BAM forward."""
        _eval_only(self)
        Cr = self.conv1.weight.shape[0]
        dummy = x.new_zeros(1)
        _, sg = F.bam_gates(x, [dummy] * 6 + self._folded(), Cr, self.dilation, channel=False, spatial=True)
        return sg.view(x.shape[0], 1, x.shape[2], x.shape[3]).expand_as(x)


class BAM(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.channel_attn = ChannelGate(channel)
        self.spatial_attn = SpatialGate(channel)

    def forward(self, x):
        _eval_only(self)
        ch, sp = self.channel_attn, self.spatial_attn
        Cr = sp.conv1.weight.shape[0]
        bn1d = F.bn_fold(ch.bn)
        params = [ch.mlp[0].weight, ch.mlp[0].bias, ch.mlp[2].weight, ch.mlp[2].bias, bn1d[0], bn1d[1]] + sp._folded()
        return F.bam_forward(x, params, Cr, sp.dilation)


class SKLayer(nn.Module):
    """attention_mechanisms/sk_module.py:17-56 (csrc/sk_dual.hip, csrc/sk_wide.hip): both grouped branches in one kernel, branch
    softmax, blend.  Takes what the reference takes: any `groups` that divides `inplanes` and `planes`, any map size H, W >= 1, fp32
    activations, eval mode; the one limit is d + planes <= 12288 (d = max(planes // ratio, 32)).  planes / groups in {1, 2, 4, 8, 16}
    runs the fp32 FMA branch kernels; every other group width (SKNet's last stage has 32, groups=1 has `planes`) runs the branches as a
    grouped implicit GEMM on the matrix cores in the fp32-class split-bf16 operand format, so results stay fp32-class for every shape
    and there is no precision switch.  mi355attn.options(sk_wide=1) sends every shape to the matrix-core kernel."""

    def __init__(self, inplanes, planes, groups=32, ratio=16):
        super().__init__()
        d = max(planes // ratio, 32)
        self.planes = planes
        self.split_3x3 = nn.Sequential(
            nn.Conv2d(inplanes, planes, kernel_size=3, padding=1, groups=groups),
            nn.BatchNorm2d(planes),
            nn.ReLU(),
        )
        self.split_5x5 = nn.Sequential(
            nn.Conv2d(inplanes, planes, kernel_size=3, padding=2, dilation=2, groups=groups),
            nn.BatchNorm2d(planes),
            nn.ReLU(),
        )
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(
            nn.Linear(planes, d),
            nn.BatchNorm1d(d),
            nn.ReLU(),
        )
        self.fc1 = nn.Linear(d, planes)
        self.fc2 = nn.Linear(d, planes)
        self.groups, self.d = groups, d

    def forward(self, x):
        _eval_only(self)
        b3 = F.bn_fold(self.split_3x3[1], self.split_3x3[0].bias)
        b5 = F.bn_fold(self.split_5x5[1], self.split_5x5[0].bias)
        bf = F.bn_fold(self.fc[1])
        params = [self.split_3x3[0].weight, b3[0], b3[1], self.split_5x5[0].weight, b5[0], b5[1],
                  self.fc[0].weight, self.fc[0].bias, bf[0], bf[1], self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]
        return F.sk_forward(x, params, self.planes, self.groups, self.d)


class PAM(nn.Module):
    """Position attention of DANet (dual_attention.py:10-28): the three 1x1 convs as ONE token-major GEMM, the streaming attention
    kernel with a single head of width `dim` and scale 1, and a transposing alpha * y + x epilogue.  The logits are unscaled dot
    products, so the default is the fp32-class precision mode (0).  Any dim from 1 to 2048 on any map size, fp32, fp16 or bf16
    activations (output in the same type; a 16-bit x takes F.conv1x1_tokens16 for the projection -- always fp32-class, x unrounded --
    and the 16-bit epilogue, `precision` selects the format of the attention core only; parameters may be 16-bit too) (_route): a head width of the streaming kernel is one head as it is; any other dim <= 256 runs zero-padded onto the next of them;
    320 / 384 / 448 / 512 (DANet itself: 512) run as two channel halves whose logits are added through the kernel's bias input;
    every other dim up to 2048 (ResNet's 2048, ViT's 768) runs zero-padded onto a multiple of 64 on the wide-head kernel, which
    contracts the logits over channel chunks and writes no hw x hw matrix."""

    _mi355_io16_core_saturates = True        # functional.range_fallback_forward: arm and wait for a 16-bit x too (q / k / v are fp32 either way)

    def __init__(self, dim):
        super().__init__()
        self.b = nn.Conv2d(dim, dim, 1)
        self.c = nn.Conv2d(dim, dim, 1)
        self.d = nn.Conv2d(dim, dim, 1)
        self.alpha = nn.Parameter(torch.zeros(1))
        self.precision = F.PREC_STRICT

    @staticmethod
    def _route(c):
        """(kind, cp): how a map of c channels runs and the head width it runs on."""
        if c in F.SDPA_WIDTHS:
            return "one", c
        if c <= F.SDPA_WIDTHS[-1]:
            return "padded", F.attn_head_width(c)
        if any(c - c0 in F.SDPA_WIDTHS for c0 in F.SDPA_WIDTHS):
            return "pair", c
        if c <= F.SDPA_WIDE_MAX:
            return "wide", (c + 63) // 64 * 64
        raise NotImplementedError(f"PAM: dim {c} is above the widest head of the attention kernels ({F.SDPA_WIDE_MAX})")

    def _fused(self, cp=None, widen=False):
        """The b | c | d weights as the rows of one GEMM and their biases, built once per parameter version.  With cp, each of the three
        blocks is zero-padded to cp rows (and bias entries): the GEMM then emits (n, hw, 3 * cp) with 16-byte aligned q / k / v slices
        for any dim; zero q / k columns add nothing to the logits, zero v columns give output columns nobody reads.  widen (the 16-bit
        activation path): the rows are built from, and cached under, the fp32 copies of 16-bit parameters (F.param32)."""
        ws = (self.b.weight, self.c.weight, self.d.weight, self.b.bias, self.c.bias, self.d.bias)
        if widen:
            ws = tuple(F.param32(t, n) for t, n in zip(ws, ("b.weight", "c.weight", "d.weight", "b.bias", "c.bias", "d.bias")))
        tag = tuple((t._version, t.data_ptr()) for t in ws)

        def build():
            w = torch.cat([t.detach() for t in ws[:3]], dim=0).contiguous()
            return F._gemm_rows(w, 0), torch.cat([t.detach() for t in ws[3:]]).contiguous()

        def build_padded():
            c = ws[0].shape[0]
            w = torch.zeros(3, cp, c, dtype=torch.float32, device=ws[0].device)
            bias = torch.zeros(3, cp, dtype=torch.float32, device=ws[0].device)
            for i in range(3):
                w[i, :c] = ws[i].detach().reshape(c, c)
                bias[i, :c] = ws[3 + i].detach()
            return F._gemm_rows(w.reshape(3 * cp, c, 1, 1), 0), bias.reshape(3 * cp)

        if cp is None:
            return F._derived_get(ws, ("pam_bcd",), tag, build)
        return F._derived_get(ws, ("pam_bcd_padded", cp), tag, build_padded)

    def forward(self, x):
        n, c, h, w = x.shape
        kind, cp = self._route(c)
        io16 = x.is_cuda and x.dtype in F._ffi.IO_CODES

        def project(rows, bias):
            if io16:
                return F.conv1x1_tokens16(x, rows, bias)
            return F.conv2d_tokens(x, None, bias, 1, 1, 0, 0, precision=self.precision, wrows=rows)[0]

        if kind in ("padded", "wide"):
            bcd = project(*self._fused(cp, widen=io16))                                                   # (n, hw, 3 cp)
            y = F.sdpa_general(bcd[:, :, :cp], bcd[:, :, cp:2 * cp], bcd[:, :, 2 * cp:], 1, 1.0, precision=self.precision)
            return F.tokens_to_nchw_axpy(y[:, :, :c], x, self.alpha)                                      # rows of cp, the first c read
        bcd = project(*self._fused(widen=io16))                                                           # (n, hw, 3c)
        q, k, v = bcd[:, :, :c], bcd[:, :, c:2 * c], bcd[:, :, 2 * c:]
        if kind == "one":
            y = F.sdpa_general(q, k, v, 1, 1.0, precision=self.precision)
        else:
            # dim above the kernel's widest head (DANet's own PAM is 512 wide): cut the channel axis in two, c = c0 + c1.  The logits
            # are a SUM over channels, q k^T = q0 k0^T + q1 k1^T, so half i attends with its own product on the matrix pipe and the
            # other half's logits (mi355_qk_logits_fwd, fp32) as the additive bias; its output is the i-th channel slice of y.
            c0 = self._split(c)
            y = torch.empty(n, h * w, c, dtype=torch.float32, device=x.device)
            for lo, hi, blo, bhi in ((0, c0, c0, c), (c0, c, 0, c0)):
                other = F.qk_logits(q[:, :, blo:bhi], k[:, :, blo:bhi], 1, precision=F.PREC_STRICT)        # (n, 1, hw, hw)
                F.sdpa_general(q[:, :, lo:hi], k[:, :, lo:hi], v[:, :, lo:hi], 1, 1.0, bias=other, precision=self.precision, out=y[:, :, lo:hi])
        return F.tokens_to_nchw_axpy(y, x, self.alpha)

    @staticmethod
    def _split(c):
        for c0 in sorted(F.SDPA_WIDTHS, reverse=True):
            if c - c0 in F.SDPA_WIDTHS:
                return c0
        raise NotImplementedError(f"PAM: dim {c} is not a sum of two head widths the attention kernel is built for {F.SDPA_WIDTHS}")


class CAM(nn.Module):
    """Channel attention of DANet (dual_attention.py:30-42).  fp32 x of any map size and channel count: where H*W or C is no multiple
    of 4 (DANet's 65 x 65 map) x is staged once into a zero-padded image in the workspace and y is stored element by element.
    fp16 / bf16 x of any shape (output in the same type, csrc/dual_attn_io16.hip): the Gram product runs on the native 16-bit matrix
    instruction (products of 16-bit values are exact in fp32) and attn . X with attn split into bf16 hi + lo, so `precision` is ignored
    for a 16-bit x: every value gives the same fp32-class result.  beta may be 16-bit too (module.half()).  An fp16 y beyond 65504 is
    inf exactly where the fp32 result rounded to fp16 is (|y| <= (1 + |beta|) max|x|); nothing is reported."""

    def __init__(self):
        super().__init__()
        self.beta = nn.Parameter(torch.zeros(1))
        self.precision = None          # operand format of attn @ x; the Gram logits always run in the fp32-class mode

    def forward(self, x):
        return F.cam_forward(x, self.beta, self.precision)
