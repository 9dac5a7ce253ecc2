"""Host-side mirror of the reference's transform modules (code/modelv2/layers.py).

Same class names, constructor arguments, parameter names (so the reference's
state_dict loads with strict=True) and NCHW tensor contract; the compute is the
HIP library.  Every transform also has a `forward_nhwc` used by
CompressionModel.forward to chain layers without leaving NHWC.

Inference only: parameters are plain tensors for the kernels, no autograd.
"""
from __future__ import annotations

import enum
import math
import os
from collections import namedtuple
from typing import NamedTuple

import torch
import torch.nn as nn

from . import lib as _lib
from . import ops

# DSIC_WINOGRAD=0 forces the direct implicit-GEMM kernel for every layer (A/B runs)
USE_WINOGRAD = os.environ.get("DSIC_WINOGRAD", "1") != "0"
# Chunk-major activations (ops.LAYOUT_CM16) between layers (A/B runs): DSIC_CHUNK_MAJOR=0 keeps every activation
# NHWC; 1 passes the first layer's output chunk-major when its consumer runs on the 64-tile Winograd kernel;
# 2 (default) also every activation whose producer and consumer both run on that kernel
CHUNK_MAJOR = int(os.environ.get("DSIC_CHUNK_MAJOR", "2"))


def wino_bf16() -> bool:
    """The library's arithmetic variant (dsic_split_bf16): True = every contraction on bf16 MFMAs with operands split
    into two bf16 planes (fp32-class results, csrc/conv_wino_bf16.hip; the default), False = fp32-input MFMAs.  One
    switch for the first layer, the Winograd layers and the image layer; DSIC_WINO_BF16=0 only sets its initial value."""
    return bool(_lib.load().dsic_split_bf16())


def set_wino_bf16(on: bool) -> None:
    """Switches the variant at run time.  Packed weights are cached per variant (_ConvBase._key), so layers built
    before the switch follow it on their next call."""
    _lib.check(_lib.load().dsic_set_split_bf16(1 if on else 0), "set_split_bf16")


def __getattr__(name):   # layers.WINO_BF16: the current variant (read-only view of the switch)
    if name == "WINO_BF16":
        return wino_bf16()
    raise AttributeError(name)


def _written(param):
    """Before a derived form of `param` (packed weights, GDN's effective beta / gamma) goes into its cache: the packers
    run on the current stream, and the cache is read from every stream the model is later called on (bench.py's lanes,
    each with a hyperprior side stream of its own) with nothing that orders those streams behind this one.  Once per
    weight version, so the host wait costs the first call only."""
    if param.is_cuda:
        torch.cuda.current_stream(param.device).synchronize()


class _GammaConv(nn.Module):
    """Holder for `gamma_conv.weight` [C,1,1,1] (layers.py:15-17)."""

    def __init__(self, channels, init):
        super().__init__()
        self.weight = nn.Parameter(init.view(channels, 1, 1, 1).clone(), requires_grad=False)


class GDN(nn.Module):
    """Diagonal GDN / IGDN (layers.py:6-27): x / sqrt(beta_c + gamma_c x^2)."""

    def __init__(self, channels, inverse=False, beta_min=1e-6, gamma_init=0.1,
                 reparam_offset=2 ** -18):
        super().__init__()
        self.inverse = inverse
        self.reparam_offset = reparam_offset
        self.beta = nn.Parameter(torch.sqrt(torch.ones(channels) + reparam_offset),
                                 requires_grad=False)
        # `gamma` [C,C] is never read by the reference's forward (layers.py:13 vs
        # :19-27); it exists only so that checkpoints load strictly.
        gamma = torch.sqrt(torch.eye(channels) * gamma_init + reparam_offset)
        self.gamma = nn.Parameter(gamma, requires_grad=False)
        self.gamma_conv = _GammaConv(channels, gamma.diag())

    def effective(self):
        """(beta_eff, gamma_eff) = (beta^2 - off, w^2 - off), layers.py:20-21.

        Cached until a parameter is rewritten or moved (load_state_dict, .to())."""
        w = self.gamma_conv.weight
        key = (self.beta._version, self.beta.data_ptr(), w._version, w.data_ptr())
        if getattr(self, "_eff_key", None) != key:
            beta = self.beta ** 2 - self.reparam_offset
            gamma = (w ** 2 - self.reparam_offset).reshape(-1)
            self._eff = (beta.contiguous(), gamma.contiguous())
            _written(w)
            self._eff_key = key
        return self._eff

    @torch.no_grad()
    def forward(self, x):
        beta, gamma = self.effective()
        return ops.gdn_nchw(x, beta, gamma, self.inverse)


class Layout(NamedTuple):
    """How an activation lies in memory.  s2d: the space-to-depth image [B,H/2,W/2,4C] of the tensor, which a 5x5/s2
    layer reads as a 3x3 conv; cm: chunk-major [B,C/16,H,W,16] (ops.LAYOUT_CM16) instead of NHWC [B,H,W,C]."""
    s2d: bool = False
    cm: bool = False


NHWC = Layout()


class Kernel(enum.Enum):
    FIRST = "first layer, from the image"
    DIRECT = "direct implicit GEMM"
    WINO_F32 = "Winograd on fp32 MFMAs"
    BF16_32 = "split-bf16 Winograd, 32 tiles"    # also its split-K form (ops.conv3x3_wino_nhwc decides) and Cout slices
    BF16_64 = "split-bf16 Winograd, 64 tiles"    # conv_wino_bf16m.hip
    IMAGE = "last layer, to the image"


class Choice(NamedTuple):
    """The kernel a layer runs on for one input (Conv2d.kernel, ConvTranspose2d.kernel) and what that launch can do
    beside plain NHWC: write its output space-to-depth; read and write chunk-major (the first layer only writes)."""
    kernel: Kernel
    s2d_out: bool = False
    cm: bool = False


def _gdn_params(gdn):
    return gdn.effective() if gdn is not None else (None, None)


_NEEDS_M64 = "chunk-major activations need the 64-tile Winograd kernel"


class _ConvBase(nn.Module):
    def __init__(self):
        super().__init__()
        self._cache, self._cache_key = {}, None

    def _key(self):
        w = self.weight
        return (w._version, w.data_ptr(), str(w.device), wino_bf16())

    def _cached(self, form, make):
        """The packed forms of the weights, each made on first use and all dropped when _key() changes."""
        key = self._key()
        if self._cache_key != key:
            self._cache, self._cache_key = {}, key
        if form not in self._cache:
            packed = make()
            _written(self.weight)
            self._cache[form] = packed
        return self._cache[form]

    def packed(self):
        return self._cached("packed", self._pack)


class Conv2d(_ConvBase):
    """nn.Conv2d(in,out,k,stride,padding=(k-1)//2) as built by conv() (layers.py:29-31)."""

    def __init__(self, in_ch, out_ch, k, stride=1):
        super().__init__()
        self.in_channels, self.out_channels = in_ch, out_ch
        self.kernel_size, self.stride = k, stride
        w = torch.empty(out_ch, in_ch, k, k)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_ch * k * k)
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_ch).uniform_(-bound, bound), requires_grad=False)

    def _pack(self):
        if self.kernel_size == 1:
            # 1x1 heads run inside dsic_hyper_params: input-major [Cin][Cout]
            return self.weight.view(self.out_channels, self.in_channels).t().contiguous()
        return ops.pack_conv_weight(self.weight)

    @property
    def use_winograd_s2(self):
        """5x5 stride-2 layers run as a 3x3 Winograd conv over the space-to-depth input (4*Cin
        channels) when the producing layer can write that layout: does this layer ask for it?"""
        # both Winograd kernels need 4*Cin as a multiple of 128 over the space-to-depth input (Cin % 32 == 0); other
        # widths (cfg.MODEL.N is configurable in the reference's train.py) take the direct implicit GEMM
        if not (USE_WINOGRAD and self.kernel_size == 5 and self.stride == 2 and self.in_channels % 32 == 0
                and self.out_channels % 4 == 0 and self.out_channels >= 64):
            return False
        # wider outputs (g_a.14: 128 -> 192, layers.py:72) run as channel slices of <= 128 into one tensor;
        # only the split-bf16 kernel can store a slice
        return self.out_channels <= 128 or (wino_bf16() and self.out_channels <= 256 and 4 * self.in_channels >= 64)

    def kernel(self, H, W, layout=NHWC, image_ch=None):
        """Which kernel runs this layer on an input of H x W pixels in `layout` (the space-to-depth grid when
        layout.s2d), and which layouts that launch can exchange.  image_ch: the input is still the image, with that
        many channels.  The only place that decides either; run_nhwc and _Chain.plan follow it."""
        cin, cout = self.in_channels, self.out_channels
        if image_ch is not None and (self.kernel_size == 3 and self.stride == 1 and cin in (3, 4) and image_ch == cin
                                     and cout <= 128 and cout % 4 == 0):
            # conv(3|4 -> <=128, 3, 1) from the NCHW image or its uint8 bytes (K = 9*Cimg, no channel padding)
            return Choice(Kernel.FIRST, s2d_out=True, cm=cout % 16 == 0)
        if layout.s2d:
            # only the Winograd kernels read space-to-depth; a layer is given it only after it asked (use_winograd_s2),
            # and one that did not ask is never given chunk-major
            cin, m64_ok = 4 * cin, self.use_winograd_s2
            if cout > 128:
                return Choice(Kernel.BF16_32)             # Cout slices of <= 128 into one NHWC tensor
        elif (USE_WINOGRAD and self.kernel_size == 3 and self.stride == 1 and cin % 32 == 0 and cout % 4 == 0
              and 64 <= cout <= 128):
            m64_ok = True                                 # 3x3 stride-1, MFMA-friendly channel counts: F(2x2,3x3)
        else:
            return Choice(Kernel.DIRECT)
        if not (wino_bf16() and cin >= 64):
            return Choice(Kernel.WINO_F32, s2d_out=True)
        if m64_ok and _lib.load().dsic_wino_bf16_m64(H, W, cin, 1):
            return Choice(Kernel.BF16_64, s2d_out=True, cm=True)
        return Choice(Kernel.BF16_32, s2d_out=True)

    def packed_wino_slices(self):
        """(lo, hi, bf16 planes) per Cout slice of at most 128, for out_channels > 128 (space-to-depth 5x5/s2).  Only
        what is made from the weight: the cache is keyed on the weight alone, so the bias is sliced at the launch."""
        def make():
            sl = []
            for lo in range(0, self.out_channels, 128):
                hi = min(lo + 128, self.out_channels)
                u = ops.pack_wino_s2_weight(self.weight[lo:hi].contiguous())
                u = ops.split_wino_weight_bf16(u, hi - lo, 4 * self.in_channels, 1)
                sl.append((lo, hi, u))
            return sl
        return self._cached("wino_slices", make)

    def packed_wino(self):
        def make():
            u = ops.pack_wino_s2_weight(self.weight) if self.kernel_size == 5 else ops.pack_wino_weight(self.weight)
            cin = self.in_channels * (4 if self.kernel_size == 5 else 1)
            if wino_bf16() and cin >= 64:
                u = ops.split_wino_weight_bf16(u, self.out_channels, cin, 1)
            return u
        return self._cached("wino", make)

    def run_nhwc(self, x, act=ops.ACT_NONE, gdn=None, x_is_s2d=False, s2d_out=False, cm_in=False, cm_out=False,
                 split_k=True):
        """x_is_s2d: x is the space-to-depth image of this layer's input; s2d_out: write the output space-to-depth;
        cm_in / cm_out: chunk-major input / output (each only where kernel() says the launch can).
        split_k: on few tiles per image, workgroups may share a tile's input channels (ops.WINO_SPLITK)."""
        B, H, W, _ = ops.cm16_shape(x) if cm_in else x.shape
        c = self.kernel(H, W, Layout(x_is_s2d, cm_in))
        assert c.cm or not (cm_in or cm_out), _NEEDS_M64
        assert c.s2d_out or not s2d_out
        beta, gamma = _gdn_params(gdn)
        if c.kernel is Kernel.DIRECT:
            return ops.conv2d_nhwc(x, self.packed(), self.bias, self.out_channels, self.kernel_size,
                                   self.stride, act, beta, gamma, cin_real=self.in_channels)
        # direct-convolution FLOPs per output channel (the space-to-depth 3x3 stands for 25 taps)
        flops = 2.0 * B * H * W * self.in_channels * (25 if x_is_s2d else 9)
        if self.out_channels > 128:
            out = torch.empty((B, H, W, self.out_channels), dtype=torch.float32, device=x.device)
            for lo, hi, u in self.packed_wino_slices():
                ops.conv3x3_wino_nhwc(x, u, self.bias[lo:hi], hi - lo, act,
                                      None if beta is None else beta[lo:hi].contiguous(),
                                      None if gamma is None else gamma[lo:hi].contiguous(), out=out, s2d_in=True,
                                      out_coff=lo, split_k=split_k, algo_flops=flops * (hi - lo))
            return out
        return ops.conv3x3_wino_nhwc(x, self.packed_wino(), self.bias, self.out_channels, act, beta, gamma,
                                     s2d_out=s2d_out, s2d_in=x_is_s2d, split_k=split_k, cm_in=cm_in, cm_out=cm_out,
                                     algo_flops=flops * self.out_channels)

    @torch.no_grad()
    def forward(self, x):
        return ops.nhwc_to_nchw(self.run_nhwc(_to_nhwc(x)))


def conv(in_ch, out_ch, k, stride=1):
    """layers.py:29-31."""
    return Conv2d(in_ch, out_ch, k, stride)


class ConvTranspose2d(_ConvBase):
    """nn.ConvTranspose2d(in,out,5,2,2,output_padding=1) (layers.py:83)."""

    def __init__(self, in_ch, out_ch, kernel_size=5, stride=2, padding=2, output_padding=1):
        super().__init__()
        if (kernel_size, stride, padding, output_padding) != (5, 2, 2, 1):
            raise ValueError("only ConvTranspose2d(k=5, s=2, p=2, output_padding=1) is on the hot path")
        self.in_channels, self.out_channels = in_ch, out_ch
        self.to_image = out_ch % 8 != 0         # the last synthesis layer: NHWC features -> NCHW image
        w = torch.empty(in_ch, out_ch, 5, 5)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(out_ch * 25)
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_ch).uniform_(-bound, bound), requires_grad=False)

    @property
    def use_winograd(self):
        return (USE_WINOGRAD and not self.to_image and self.in_channels % 32 == 0
                and self.out_channels % 4 == 0 and 64 <= self.out_channels <= 128)

    def _pack(self):
        if self.to_image:
            return ops.pack_convT_image_weight(self.weight)
        if self.use_winograd:
            u = ops.pack_wino_convT_weight(self.weight)
            if wino_bf16() and self.in_channels >= 64:
                u = ops.split_wino_weight_bf16(u, self.out_channels, self.in_channels, 4)
            return u
        return ops.pack_convT_weight(self.weight)

    def kernel(self, H, W, layout=NHWC):
        """Which kernel runs this layer on an H x W input, and which layouts that launch can exchange (see
        Conv2d.kernel): no transposed form reads or writes space-to-depth, the image layer takes NHWC only."""
        assert not layout.s2d
        if self.to_image:
            return Choice(Kernel.IMAGE)
        if not self.use_winograd:
            return Choice(Kernel.DIRECT)
        if not (wino_bf16() and self.in_channels >= 64):
            return Choice(Kernel.WINO_F32)
        if _lib.load().dsic_wino_bf16_m64(H, W, self.in_channels, 4):
            return Choice(Kernel.BF16_64, cm=True)
        return Choice(Kernel.BF16_32)

    def run_nhwc(self, x, act=ops.ACT_NONE, gdn=None, cm_in=False, cm_out=False):
        _, H, W, _ = ops.cm16_shape(x) if cm_in else x.shape
        c = self.kernel(H, W, Layout(cm=cm_in))
        assert c.cm or not (cm_in or cm_out), _NEEDS_M64
        if c.kernel is Kernel.IMAGE:   # returns NCHW image
            return ops.conv_transpose2d_image(x, self.packed(), self.bias, self.out_channels)
        beta, gamma = _gdn_params(gdn)
        if c.kernel is Kernel.DIRECT:
            return ops.conv_transpose2d_nhwc(x, self.packed(), self.bias, self.out_channels, act, beta, gamma)
        return ops.conv_transpose2d_wino_nhwc(x, self.packed(), self.bias, self.out_channels, act, beta, gamma,
                                              cm_in=cm_in, cm_out=cm_out)

    @torch.no_grad()
    def forward(self, x):
        y = self.run_nhwc(_to_nhwc(x))
        return y if self.to_image else ops.nhwc_to_nchw(y)


def _f32_image(x):
    if x.dim() != 4:
        raise ValueError(f"expected [N,C,H,W], got {tuple(x.shape)}")
    return x


def _to_nhwc(x):
    """NCHW -> NHWC with the channel count padded to a multiple of 8."""
    if x.dim() != 4:
        raise ValueError(f"expected [N,C,H,W], got {tuple(x.shape)}")
    C = x.shape[1]
    if C <= 8 and C % 8 != 0:
        return ops.image_to_nhwc8(x)
    if C % 8 != 0:
        raise ValueError(f"channel count {C} must be <= 8 or a multiple of 8")
    return ops.nchw_to_nhwc(x)


# One launch of a chain's plan: the conv (or a GDN | nn.ReLU that no conv takes in: kernel None), the activation fused
# into its kernel (ops.ACT_*) with its GDN or None, the Layouts it reads and writes, and the Kernel
Step = namedtuple("Step", "conv act gdn lay_in lay_out kernel")


def _fused(nxt, kernel):
    """(act, gdn, modules consumed): the activation after a conv that its kernel applies itself."""
    if isinstance(nxt, GDN) and not (nxt.inverse and kernel is Kernel.FIRST):
        return (ops.ACT_IGDN if nxt.inverse else ops.ACT_GDN), nxt, 2
    if isinstance(nxt, nn.ReLU):
        return ops.ACT_RELU, None, 2
    return ops.ACT_NONE, None, 1


class _Chain(nn.Sequential):
    """nn.Sequential whose (conv, GDN|ReLU) pairs run as one fused kernel, in the layouts plan() chooses."""

    def __init__(self, *mods, split_k=True):
        super().__init__(*mods)
        # HyperAnalysis switches split-K off: its launches run on the side stream, where every extra launch waits for
        # compute units at a kernel boundary of the main stream
        self.split_k = split_k

    def plan(self, shape, dtype, from_image=False):
        """The launches of this chain for an input of `shape` and `dtype`: NHWC activations, or with from_image the
        NCHW float32 image or its uint8 [B,H,W,C] bytes.  Pure: no tensors, no launches, recomputed on every call.

        An edge between two layers is space-to-depth when the consumer asks for it (Conv2d.use_winograd_s2, even
        sizes) and the producer's launch can write it; chunk-major when the consumer then runs on the 64-tile
        Winograd kernel and the producer is the first layer (CHUNK_MAJOR >= 1) or that kernel too (CHUNK_MAJOR >= 2).
        The chain's input and output are always NHWC (or the image)."""
        mods = list(self)
        if from_image and dtype != torch.uint8:
            shape = shape[0], shape[2], shape[3], shape[1]
        (_, H, W, C), steps, lay, i = shape, [], NHWC, 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, (GDN, nn.ReLU)):            # no conv before it to be fused into
                assert lay == NHWC
                steps.append(Step(m, ops.ACT_NONE, None, NHWC, NHWC, None))
                i += 1
                continue
            if isinstance(m, Conv2d):
                c = m.kernel(H, W, lay, C if from_image and i == 0 else None)
                Ho, Wo = (H, W) if lay.s2d else (-(-H // m.stride), -(-W // m.stride))
            elif isinstance(m, ConvTranspose2d):
                c = m.kernel(H, W, lay)
                Ho, Wo = 2 * H, 2 * W
            else:
                raise TypeError(f"unsupported module {type(m).__name__}")
            act, gdn, n = _fused(mods[i + 1] if i + 1 < len(mods) else None, c.kernel)
            i += n
            con = mods[i] if i < len(mods) else None     # the consumer of this launch's output
            s2d = isinstance(con, Conv2d) and con.use_winograd_s2 and Ho % 2 == 0 and Wo % 2 == 0
            # the Cout-slice form reads space-to-depth but cannot write it: such a chain is refused, not run NHWC
            assert c.s2d_out or not (s2d and lay.s2d)
            s2d = s2d and c.s2d_out
            Ho, Wo = (Ho // 2, Wo // 2) if s2d else (Ho, Wo)
            cm = (c.cm and CHUNK_MAJOR >= (1 if c.kernel is Kernel.FIRST else 2)
                  and isinstance(con, (Conv2d, ConvTranspose2d)) and con.kernel(Ho, Wo, Layout(s2d)).cm)
            steps.append(Step(m, act, gdn, lay, Layout(s2d, cm), c.kernel))
            H, W, lay = Ho, Wo, Layout(s2d, cm)
        assert lay == NHWC
        return steps

    def _run(self, steps, x, taps):
        for st in steps:
            m, i, o = st.conv, st.lay_in, st.lay_out
            if st.kernel is None:
                x = torch.relu(x) if isinstance(m, nn.ReLU) else ops.nchw_to_nhwc(m(ops.nhwc_to_nchw(x)))
            elif st.kernel is Kernel.FIRST:
                x = ops.conv_first_nchw(x, m.weight, m.bias, st.act, *_gdn_params(st.gdn), s2d_out=o.s2d, cm_out=o.cm)
            elif isinstance(m, Conv2d):
                x = m.run_nhwc(x, st.act, st.gdn, i.s2d, o.s2d, i.cm, o.cm, self.split_k)
            else:
                x = m.run_nhwc(x, st.act, st.gdn, i.cm, o.cm)
            if taps is not None:
                # a tap in the layout the fixtures know: NHWC at the layer's own resolution
                t = ops.cm16_to_nhwc(x) if o.cm else x
                taps.append(ops.depth_to_space(t) if o.s2d else t)
        return x

    def forward_from_image(self, x_nchw, taps=None):
        """Like forward_nhwc but from an NCHW image, or from decoded image bytes (uint8 [B,H,W,C]: to_tensor is fused
        into the first-layer kernel)."""
        steps = self.plan(x_nchw.shape, x_nchw.dtype, from_image=True)
        if not (steps and steps[0].kernel is Kernel.FIRST):
            x_nchw = _to_nhwc(ops.to_tensor_u8(x_nchw) if x_nchw.dtype == torch.uint8 else x_nchw)
        return self._run(steps, x_nchw, taps)

    def forward_nhwc(self, x, taps=None):
        """NHWC in, NHWC (or the NCHW image) out; taps: a list that receives every launch's output."""
        return self._run(self.plan(x.shape, x.dtype), x, taps)

    @torch.no_grad()
    def forward(self, x):
        y = self.forward_nhwc(_to_nhwc(x))
        last = list(self)[-1]
        return y if isinstance(last, ConvTranspose2d) and last.to_image else ops.nhwc_to_nchw(y)


class AnalysisTransform(nn.Module):
    """layers.py:46-76: 8 convs (3/1,5/2 alternating) + 7 GDN, /16."""

    def __init__(self, N=128, M=192, in_ch=3):
        super().__init__()
        self.g_a = _Chain(
            conv(in_ch, N, 3, 1), GDN(N),
            conv(N, N, 5, 2), GDN(N),
            conv(N, N, 3, 1), GDN(N),
            conv(N, N, 5, 2), GDN(N),
            conv(N, N, 3, 1), GDN(N),
            conv(N, N, 5, 2), GDN(N),
            conv(N, N, 3, 1), GDN(N),
            conv(N, M, 5, 2),
        )

    def forward_nhwc(self, x, taps=None):
        return self.g_a.forward_nhwc(x, taps)

    def forward_from_image(self, x_nchw, taps=None):
        return self.g_a.forward_from_image(x_nchw, taps)

    def forward(self, x):
        return ops.nhwc_to_nchw(self.g_a.forward_from_image(_f32_image(x)))


class SynthesisTransform(nn.Module):
    """layers.py:78-101: 4 convT + 3 conv + 6 IGDN, x16."""

    def __init__(self, N=128, M=192, out_ch=3):
        super().__init__()
        self.g_s = _Chain(
            ConvTranspose2d(M, N, 5, 2, 2, output_padding=1), GDN(N, inverse=True),
            conv(N, N, 3, 1), GDN(N, inverse=True),
            ConvTranspose2d(N, N, 5, 2, 2, output_padding=1), GDN(N, inverse=True),
            conv(N, N, 3, 1), GDN(N, inverse=True),
            ConvTranspose2d(N, N, 5, 2, 2, output_padding=1), GDN(N, inverse=True),
            conv(N, N, 3, 1), GDN(N, inverse=True),
            ConvTranspose2d(N, out_ch, 5, 2, 2, output_padding=1),
        )

    def forward_nhwc(self, y_hat, taps=None):
        """NHWC latents -> NCHW image."""
        return self.g_s.forward_nhwc(y_hat, taps)

    def forward(self, y_hat):
        return self.g_s(y_hat)


class HyperAnalysis(nn.Module):
    """layers.py:104-116."""

    def __init__(self, M=192, N=128):
        super().__init__()
        self.h_a = _Chain(
            conv(M, N, 3, 1), nn.ReLU(inplace=True),
            conv(N, N, 3, 1), nn.ReLU(inplace=True),
            conv(N, N, 5, 2), nn.ReLU(inplace=True),
            conv(N, N, 5, 2),
            split_k=False,
        )

    def forward_nhwc(self, y, taps=None):
        return self.h_a.forward_nhwc(y, taps)

    def forward(self, y):
        return self.h_a(y)


class HyperSynthesis(nn.Module):
    """layers.py:118-152, non-spatial heads (the only branch any reference script uses)."""

    def __init__(self, N=128, M=128, spatial_params=False):
        super().__init__()
        self.spatial_params = spatial_params
        self.N, self.M = N, M
        self.h_s = _Chain(
            ConvTranspose2d(N, N, 5, 2, 2, output_padding=1), nn.ReLU(inplace=True),
            ConvTranspose2d(N, N, 5, 2, 2, output_padding=1), nn.ReLU(inplace=True),
        )
        if spatial_params:      # layers.py:127-129: per-element heads
            self.to_sigma = conv(N, M, 3, 1)
            self.to_nu = conv(N, M, 3, 1)
        else:                   # layers.py:130-139: global per-channel heads
            self.pool = nn.AdaptiveAvgPool2d(1)
            self.mlp_sigma = nn.Sequential(Conv2d(N, N, 1), nn.ReLU(), Conv2d(N, M, 1))
            self.mlp_nu = nn.Sequential(Conv2d(N, N, 1), nn.ReLU(), Conv2d(N, M, 1))

    def params_nhwc(self, z_hat_nhwc, min_nu, max_nu, taps=None):
        """spatial_params=False: -> ((log_sigma, log_nu, sigma, nu) each [B,M], (Ht, Wt)).
        spatial_params=True:  -> ((log_sigma, log_nu) NHWC [B,Ht,Wt,M], sigma, nu NCHW), (Ht, Wt)."""
        t = self.h_s.forward_nhwc(z_hat_nhwc, taps)
        if self.spatial_params:
            ls = self.to_sigma.run_nhwc(t)
            ln = self.to_nu.run_nhwc(t)
            sigma, nu = ops.sigma_nu_spatial(ls, ln, min_nu, max_nu)
            return (ls, ln, sigma, nu), (t.shape[1], t.shape[2])
        s0, s2 = self.mlp_sigma[0], self.mlp_sigma[2]
        n0, n2 = self.mlp_nu[0], self.mlp_nu[2]
        outs = ops.hyper_params(t, s0.packed(), s0.bias, s2.packed(), s2.bias, n0.packed(), n0.bias,
                                n2.packed(), n2.bias, self.M, min_nu, max_nu)
        return outs, (t.shape[1], t.shape[2])

    @torch.no_grad()
    def forward(self, z):
        # clamp bounds are irrelevant for the log outputs returned here
        (log_sigma, log_nu, _, _), (Ht, Wt) = self.params_nhwc(_to_nhwc(z), 0.0, float("inf"))
        if self.spatial_params:
            return ops.nhwc_to_nchw(log_sigma), ops.nhwc_to_nchw(log_nu)
        B = z.shape[0]
        return (log_sigma.view(B, self.M, 1, 1).expand(-1, -1, Ht, Wt),
                log_nu.view(B, self.M, 1, 1).expand(-1, -1, Ht, Wt))
