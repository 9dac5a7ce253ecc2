"""Thin torch-tensor wrappers over the C ABI (device pointers + current stream).

PyTorch is plumbing here: it owns device memory and the HIP stream; every
function forwards raw pointers to libdsic_hip.so.
"""
from __future__ import annotations

import ctypes
import operator
import os

import numpy as np
import torch

from . import lib as _lib
from .lib import ACT_GDN, ACT_IGDN, ACT_NONE, ACT_RELU  # noqa: F401


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    # one process drives one GPU (torch.distributed, one rank per device): the current stream of the
    # current device.  Tensors on another device are rejected by _f32c's callers' pointer checks.
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _int_option(value, name, top, what, note="") -> int:
    """An integer option of the image codec (nodata, fill, max_error, tolerance): value as an int in 0 .. top, else
    ValueError.  A bool, NumPy's included, is no integer here."""
    try:
        v = -1 if isinstance(value, (bool, np.bool_)) else operator.index(value)
    except TypeError:
        v = -1
    if not 0 <= v <= top:
        raise ValueError(f"{what}: {name}={value!r} must be an integer from 0{note} to {top}")
    return v


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the GPU (no CPU fallback), got {t.device}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.device.index != torch.cuda.current_device():
        # launches go to the current stream of the current device (_stream): a tensor of another GPU would be
        # read through the wrong stream, and its kernel attributes are set per device
        raise RuntimeError(f"{name}: tensor on {t.device}, current device is cuda:{torch.cuda.current_device()} "
                           "(one process drives one GPU; wrap the call in torch.cuda.device(...))")
    return t.contiguous()


# DSIC_WINO_SPLITK=0: never share a tile's input channels between workgroups (dsic_wino_bf16_ksplit decides otherwise)
WINO_SPLITK = os.environ.get("DSIC_WINO_SPLITK", "1") != "0"

# Optional per-launch timer (bench.py): object with .record(tag, flops, launch)
# where launch() enqueues the kernel on the current stream.
_kernel_timer = None


def set_kernel_timer(timer):
    global _kernel_timer
    _kernel_timer = timer


def _conv_kernel_name(win, stride, Wo, Cin, CoutP, Ho=None, B=None, nphase=1):
    """Template instantiation conv_igemm.hip dispatches to (for profile matching).  Ho, B, nphase (4 for the
    transposed conv): the workgroup count that decides between two column tiles per wave and column blocks for
    CoutP > 128 (run_conv_ck); without them the grid is taken to be large."""
    ck = (32 if Cin % 32 == 0 else 8) if win == 3 else (16 if Cin % 16 == 0 else 8)
    if Wo > 8:
        tile = (16, 8, 1)
    elif Wo > 4:
        tile = (8, 8, 2)
    else:
        tile = (4, 4, 8)
        if win == 5:
            ck = 8
    nt = CoutP // 32
    ntw, narrow = (1, 1) if nt == 1 else ((1, 0) if nt <= 4 else (2, 0))
    if ntw == 2 and Ho is not None and B is not None:
        wgs = -(-Wo // tile[0]) * -(-Ho // tile[1]) * -(-B // tile[2]) * nphase
        if wgs < 512:
            ntw = 1                                     # columns split over blockIdx.z instead
    return f"conv_igemm_kernel<{win},{stride},{tile[0]},{tile[1]},{tile[2]},{ck},{ntw},{narrow}>"


def _timed(name, flops, launch, exec_flops=None):
    """flops: algorithmic (direct-convolution) FLOPs of the launch; exec_flops: FLOPs the MFMA
    pipe actually executes (smaller for Winograd, larger where channels are padded)."""
    if _kernel_timer is None:
        return launch()
    return _kernel_timer.record(name, flops, launch, exec_flops if exec_flops is not None else flops)


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _pack(name, w, k, size, call, dtype=torch.float32):
    """One weight packer: w [C0,C1,k,k] (k None: any square kernel) -> size(L, C0, C1, k) elements of dtype on w's
    device, written by call(L, pointer to w, pointer to them, C0, C1, k)."""
    w = _f32c(w, name)
    C0, C1, kh, kw = w.shape
    if k is None:
        assert kh == kw
    elif (kh, kw) != (k, k):
        raise ValueError(f"{name}: kernel must be {k}x{k}")
    L = _lib.load()
    dst = torch.empty(size(L, C0, C1, kh), dtype=dtype, device=w.device)
    _lib.check(call(L, _p(w), _p(dst), C0, C1, kh), name)
    return dst


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d weight [Cout,Cin,k,k] -> [k*k][CinP/8][CoutP][8]."""
    return _pack("pack_conv_weight", w, None, lambda L, Cout, Cin, k: L.dsic_packed_conv_weight_floats(Cout, Cin, k),
                 lambda L, w, dst, Cout, Cin, k: L.dsic_pack_conv_weight(w, dst, Cout, Cin, k, _stream()))


def pack_convT_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.ConvTranspose2d weight [Cin,Cout,5,5] -> four phase kernels, 25 taps."""
    return _pack("pack_convT_weight", w, 5, lambda L, Cin, Cout, k: 25 * (Cin // 8) * round_up(Cout, 32) * 8,
                 lambda L, w, dst, Cin, Cout, k: L.dsic_pack_convT_weight(w, dst, Cin, Cout, _stream()))


def pack_convT_image_weight(w: torch.Tensor) -> torch.Tensor:
    def size(L, Cin, Cimg, k):
        if Cin % 16 or not 1 <= Cimg <= 4:
            raise ValueError("pack_convT_image_weight: Cin must be a multiple of 16 and Cimg in [1,4]")
        return L.dsic_convT_image_weight_floats(Cin)
    return _pack("pack_convT_image_weight", w, 5, size,
                 lambda L, w, dst, Cin, Cimg, k: L.dsic_pack_convT_image_weight(w, dst, Cin, Cimg, _stream()))


def image_to_nhwc8(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "image_to_nhwc8")
    B, C, H, W = x.shape
    dst = torch.empty((B, H, W, 8), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dsic_image_to_nhwc8(_p(x), _p(dst), B, C, H, W, _stream()), "image_to_nhwc8")
    return dst


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "nhwc_to_nchw")
    B, H, W, C = x.shape
    dst = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dsic_nhwc_to_nchw(_p(x), _p(dst), B, H, W, C, _stream()), "nhwc_to_nchw")
    return dst


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "nchw_to_nhwc")
    B, C, H, W = x.shape
    dst = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dsic_nchw_to_nhwc(_p(x), _p(dst), B, C, H, W, _stream()), "nchw_to_nhwc")
    return dst


def conv2d_nhwc(x, w_packed, bias, Cout, k, stride, act=ACT_NONE, beta=None, gamma=None, out=None,
                cin_real=None):
    """conv() + fused activation on NHWC activations (layers.py:29-31)."""
    x = _f32c(x, "conv2d_nhwc")
    B, H, W, CinP = x.shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    _timed(_conv_kernel_name(k, stride, Wo, CinP, round_up(Cout, 32), Ho, B),
           2.0 * B * Ho * Wo * Cout * (cin_real or CinP) * k * k,
           lambda: _lib.check(L.dsic_conv2d_nhwc(_p(x), _p(w_packed), _p(bias), _p(beta), _p(gamma),
                                                 _p(out), B, H, W, CinP, Cout, k, stride, act, _stream()),
                              "conv2d_nhwc"))
    return out


def pack_wino_weight(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d 3x3 weight [Cout,Cin,3,3] -> Winograd-domain U = G g G^T, [16][Cin/8][CoutP][8]."""
    return _pack("pack_wino_weight", w, 3, lambda L, Cout, Cin, k: L.dsic_wino_weight_floats(Cout, Cin),
                 lambda L, w, dst, Cout, Cin, k: L.dsic_pack_wino_weight(w, dst, Cout, Cin, _stream()))


def pack_wino_s2_weight(w: torch.Tensor) -> torch.Tensor:
    """5x5 stride-2 weight [Cout,Cs,5,5] -> Winograd U of the equivalent 3x3 conv over 4*Cs s2d channels."""
    return _pack("pack_wino_s2_weight", w, 5, lambda L, Cout, Cs, k: L.dsic_wino_weight_floats(Cout, 4 * Cs),
                 lambda L, w, dst, Cout, Cs, k: L.dsic_pack_wino_s2_weight(w, dst, Cout, Cs, _stream()))


_tickets = {}


def _ticket(device):
    """16 zeroed bytes per (device, stream): the persistent Winograd kernel's tile ticket."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _tickets.get(key)
    if t is None:
        t = torch.zeros(2, dtype=torch.int64, device=device)
        _tickets[key] = t
    return t


def pack_wino_convT_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d weight [Cin,Cout,5,5] -> Winograd U of its four 3x3 sub-pixel phase convs."""
    return _pack("pack_wino_convT_weight", w, 5, lambda L, Cin, Cout, k: 4 * L.dsic_wino_weight_floats(Cout, Cin),
                 lambda L, w, dst, Cin, Cout, k: L.dsic_pack_wino_convT_weight(w, dst, Cin, Cout, _stream()))


def split_wino_weight_bf16(u_f32: torch.Tensor, Cout: int, Cin: int, nphase: int = 1) -> torch.Tensor:
    """fp32 transformed weights (pack_wino_*_weight) -> bf16 planes for the *_wino_bf16 kernels (uint8 tensor)."""
    L = _lib.load()
    dst = torch.empty(nphase * L.dsic_wino_bf16_weight_bytes(Cout, Cin), dtype=torch.uint8, device=u_f32.device)
    _lib.check(L.dsic_split_wino_weight_bf16(_p(u_f32), _p(dst), Cout, Cin, nphase, _stream()), "split_wino_weight_bf16")
    return dst


def wino_bf16_planes() -> int:
    return int(_lib.load().dsic_wino_bf16_planes())


def _wino_exec_flops(tiles, positions, nprod, Cin, CoutP):
    """FLOPs the MFMA pipe executes in a Winograd launch: `tiles` 2x2-output tiles (border padding included) of
    `positions` live Winograd positions (16; 12.25 on average with a space-to-depth input or the phases of a
    transposed layer), `nprod` bf16 products per position (1: the fp32 kernel), Cin x CoutP each."""
    return 2.0 * nprod * tiles * positions * Cin * CoutP


def _wino_bf16_products():
    return 3 if wino_bf16_planes() == 2 else 6


def conv_transpose2d_wino_nhwc(x, u_packed4, bias, Cout, act=ACT_NONE, beta=None, gamma=None, out=None,
                               cm_in=False, cm_out=False):
    """ConvTranspose2d(Cin,Cout,5,2,2,1) + fused activation: four Winograd 3x3 phase convs.
    u_packed4: fp32 transformed weights (fp32 MFMA kernel) or the uint8 bf16 planes of
    split_wino_weight_bf16 (split-bf16 kernel).  cm_in / cm_out: the input / output is chunk-major
    [B,C/16,H,W,16] (nhwc_to_cm16; layers of the 64-tile kernel only)."""
    x = _f32c(x, "conv_transpose2d_wino_nhwc")
    B, H, W, Cin = cm16_shape(x) if cm_in else x.shape
    if out is None:
        out = torch.empty(_act_shape(B, 2 * H, 2 * W, Cout, cm_out), dtype=torch.float32, device=x.device)
    L = _lib.load()
    wino_tiles = 4 * B * (-(-H // 8)) * (-(-W // 16)) * 32

    def args(*layouts):
        return (_p(x), _p(u_packed4), _p(bias), _p(beta), _p(gamma), _p(out), B, H, W, Cin, Cout, act, *layouts,
                _p(_ticket(x.device)), _stream())
    if u_packed4.dtype == torch.uint8:
        nprod = _wino_bf16_products()
        # large layers run on the 64-tile two-pass kernel (conv_wino_bf16m.hip): the symbol the profiler will show
        name = "conv_wino_bf16m_kernel<2>" if L.dsic_wino_bf16_m64(H, W, Cin, 4) else "conv_wino_bf16_kernel<2>"
        what, call = "conv_transpose2d_wino_bf16_layout", lambda: L.dsic_conv_transpose2d_wino_bf16_layout(
            *args(LAYOUT_CM16 if cm_in else 0, LAYOUT_CM16 if cm_out else 0))
    elif cm_in or cm_out:
        raise ValueError("conv_transpose2d_wino_nhwc: chunk-major activations need the split-bf16 kernel")
    else:
        nprod, name = 1, "conv_wino_kernel<2>"
        what, call = "conv_transpose2d_wino_nhwc", lambda: L.dsic_conv_transpose2d_wino_nhwc(*args())
    _timed(name, 2.0 * B * H * W * Cout * Cin * 25, lambda: _lib.check(call(), what),
           exec_flops=_wino_exec_flops(wino_tiles, 12.25, nprod, Cin, round_up(Cout, 32)))
    return out


def space_to_depth(x_nhwc):
    """[B,H,W,C] -> [B,H/2,W/2,4C] with channel (a*2+b)*C+c = x[2i+a][2j+b][c] (layout plumbing)."""
    B, H, W, C = x_nhwc.shape
    return x_nhwc.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C).contiguous()


def depth_to_space(x_s2d):
    B, H2, W2, C4 = x_s2d.shape
    C = C4 // 4
    return x_s2d.view(B, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C).contiguous()


# Chunk-major activations (CM16, DSIC_LAYOUT_CM16 in include/dsic_hip.h): [B][C/16][H][W][16] fp32, the channel axis
# of the NHWC tensor cut into 16-channel chunks, each a contiguous plane.  Written by a producer whose consumer runs
# on the 64-tile Winograd kernel (layers._Chain decides); these conversions are layout plumbing for taps and tests.
LAYOUT_CM16 = 2


def cm16_shape(x_cm):
    """(B, H, W, C) of a chunk-major tensor."""
    B, CC, H, W, K = x_cm.shape
    assert K == 16, tuple(x_cm.shape)
    return B, H, W, 16 * CC


def _act_shape(B, H, W, C, cm):
    return (B, C // 16, H, W, 16) if cm else (B, H, W, C)


def _out_shape(B, H, W, Cout, s2d_out, cm_out):
    """Output of a stride-1 layer over [B,H,W,.]: stored space-to-depth it is [B,H/2,W/2,4*Cout]."""
    return _act_shape(B, H // 2, W // 2, 4 * Cout, cm_out) if s2d_out else _act_shape(B, H, W, Cout, cm_out)


def cm16_to_nhwc(x_cm):
    B, H, W, C = cm16_shape(x_cm)
    return x_cm.permute(0, 2, 3, 1, 4).reshape(B, H, W, C).contiguous()


def nhwc_to_cm16(x_nhwc):
    B, H, W, C = x_nhwc.shape
    return x_nhwc.view(B, H, W, C // 16, 16).permute(0, 3, 1, 2, 4).contiguous()


def conv3x3_wino_nhwc(x, u_packed, bias, Cout, act=ACT_NONE, beta=None, gamma=None, out=None, s2d_out=False,
                      algo_flops=None, s2d_in=False, out_coff=0, split_k=True, cm_in=False, cm_out=False):
    """conv(Cin,Cout,3,1) + fused activation by Winograd F(2x2,3x3) on NHWC activations.

    s2d_out: write [B,H/2,W/2,4*Cout] (space-to-depth) for a following 5x5/s2 layer.
    cm_in / cm_out: the input / output is chunk-major [B,C/16,H,W,16] (layers of the 64-tile kernel only)."""
    x = _f32c(x, "conv3x3_wino_nhwc")
    B, H, W, Cin = cm16_shape(x) if cm_in else x.shape
    if out is None:
        out = torch.empty(_out_shape(B, H, W, Cout, s2d_out, cm_out), dtype=torch.float32, device=x.device)
    L = _lib.load()
    wino_tiles = B * (-(-H // 8)) * (-(-W // 16)) * 32          # 2x2-output tiles incl. border padding
    bf16 = u_packed.dtype == torch.uint8                         # bf16 planes: split-bf16 kernel
    if (cm_in or cm_out) and not bf16:
        raise ValueError("conv3x3_wino_nhwc: chunk-major activations need the split-bf16 kernel")
    mode, s2d_o, s2d_i = (1 if s2d_in else 0), int(bool(s2d_out)), int(bool(s2d_in))

    def args(*rest):
        return (_p(x), _p(u_packed), _p(bias), _p(beta), _p(gamma), _p(out), B, H, W, Cin, Cout, act, *rest,
                _p(_ticket(x.device)), _stream())
    ksplit = L.dsic_wino_bf16_ksplit(H, W, Cin) if (bf16 and WINO_SPLITK and split_k) else 1
    if not bf16:
        name = f"conv_wino_kernel<{mode}>"
        what, call = "conv3x3_wino_nhwc", lambda: L.dsic_conv3x3_wino_nhwc(*args(s2d_o, s2d_i))
    elif ksplit > 1 and not (cm_in or cm_out):
        # few tiles per image: the input channels of a tile are shared by `ksplit` work items
        partials = torch.empty((ksplit,) + tuple(out.shape), dtype=torch.float32, device=x.device)
        name = f"conv_wino_bf16_kernel<{mode}>"
        what, call = "conv3x3_wino_bf16_splitk_nhwc", lambda: L.dsic_conv3x3_wino_bf16_splitk_nhwc(*args(
            s2d_o, s2d_i, 0 if s2d_out else int(out.shape[-1]), int(out_coff), ksplit, _p(partials)))
    else:
        m64 = "m" if L.dsic_wino_bf16_m64(H, W, Cin, 1) else ""   # 64-tile two-pass kernel (conv_wino_bf16m.hip)
        name = f"conv_wino_bf16{m64}_kernel<{mode}>"
        what, call = "conv3x3_wino_bf16_nhwc", lambda: L.dsic_conv3x3_wino_bf16_nhwc(*args(
            s2d_o | (LAYOUT_CM16 if cm_out else 0), s2d_i | (LAYOUT_CM16 if cm_in else 0),
            0 if (s2d_out or cm_out) else int(out.shape[-1]), int(out_coff)))
    _timed(name, algo_flops if algo_flops is not None else 2.0 * B * H * W * Cout * Cin * 9,
           lambda: _lib.check(call(), what),
           exec_flops=_wino_exec_flops(wino_tiles, 12.25 if s2d_in else 16, _wino_bf16_products() if bf16 else 1, Cin,
                                       round_up(Cout, 32)))
    return out


def to_tensor_u8(x_u8_nhwc: torch.Tensor) -> torch.Tensor:
    """torchvision to_tensor (modelseval.py:66-67): uint8 [B,H,W,C] on the GPU -> float32 [B,C,H,W] in [0,1]."""
    if not x_u8_nhwc.is_cuda or x_u8_nhwc.dtype != torch.uint8 or x_u8_nhwc.dim() != 4:
        raise TypeError("to_tensor_u8: expected a uint8 [B,H,W,C] tensor on the GPU")
    x = x_u8_nhwc.contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dsic_image_u8hwc_to_f32nchw(_p(x), _p(out), B, C, H, W, _stream()), "to_tensor_u8")
    return out


def conv_first_nchw(x, w, bias, act=ACT_NONE, beta=None, gamma=None, s2d_out=False, cm_out=False):
    """conv(Cimg,Cout,3,1) + fused activation from the image to NHWC (layers.py:51).
    x: float32 NCHW in [0,1] (the reference's tensor contract), or uint8 NHWC image bytes
    (to_tensor fused into the kernel).  cm_out: write the output chunk-major [B,C/16,H',W',16]."""
    w = _f32c(w, "conv_first_nchw")
    Cout = w.shape[0]
    flag = int(bool(s2d_out)) | (LAYOUT_CM16 if cm_out else 0)
    if x.dtype == torch.uint8:
        if not x.is_cuda:
            raise RuntimeError(f"conv_first_nchw: expected a tensor on the GPU (no CPU fallback), got {x.device}")
        x, what = x.contiguous(), "conv_first_u8hwc"
        B, H, W, C = x.shape
    else:
        x, what = _f32c(x, "conv_first_nchw"), "conv_first_nchw"
        B, C, H, W = x.shape
    out = torch.empty(_out_shape(B, H, W, Cout, s2d_out, cm_out), dtype=torch.float32, device=x.device)
    fn = getattr(_lib.load(), "dsic_" + what)
    _timed(f"conv_first_kernel<{C}>", 2.0 * B * H * W * Cout * C * 9,
           lambda: _lib.check(fn(_p(x), _p(w), _p(bias), _p(beta), _p(gamma), _p(out), B, C, H, W, Cout, act, flag,
                                 _stream()), what))
    return out


def conv_transpose2d_nhwc(x, w_packed, bias, Cout, act=ACT_NONE, beta=None, gamma=None, out=None):
    """ConvTranspose2d(Cin,Cout,5,2,2,output_padding=1) + fused activation."""
    x = _f32c(x, "conv_transpose2d_nhwc")
    B, H, W, Cin = x.shape
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, Cout), dtype=torch.float32, device=x.device)
    L = _lib.load()
    _timed(_conv_kernel_name(3, 1, W, Cin, round_up(Cout, 32), H, B, 4),
           2.0 * B * H * W * Cout * Cin * 25,
           lambda: _lib.check(L.dsic_conv_transpose2d_nhwc(_p(x), _p(w_packed), _p(bias), _p(beta),
                                                           _p(gamma), _p(out), B, H, W, Cin, Cout, act,
                                                           _stream()), "conv_transpose2d_nhwc"))
    return out


def conv_transpose2d_image(x, w_packed, bias, Cimg, out=None):
    """Last synthesis layer: NHWC features -> NCHW image [B,Cimg,2H,2W]."""
    x = _f32c(x, "conv_transpose2d_image")
    B, H, W, Cin = x.shape
    if out is None:
        out = torch.empty((B, Cimg, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    L = _lib.load()
    _timed("convT_image_kernel", 2.0 * B * H * W * Cimg * Cin * 25,
           lambda: _lib.check(L.dsic_conv_transpose2d_image(_p(x), _p(w_packed), _p(bias), _p(out), B, H, W,
                                                            Cin, Cimg, _stream()), "conv_transpose2d_image"),
           exec_flops=2.0 * B * (-(-H // 16) * 16) * (-(-W // 32) * 32) * 16 * Cin * 9)
    return out


def round_half_even(x: torch.Tensor) -> torch.Tensor:
    """quantize(x, "round") (model.py:32-33)."""
    x = _f32c(x, "round")
    out = torch.empty_like(x)
    _lib.check(_lib.load().dsic_round(_p(x), _p(out), x.numel(), _stream()), "round")
    return out


def gdn_nchw(x, beta_eff, gamma_eff, inverse: bool):
    """Stand-alone GDN / IGDN on NCHW (layers.py:19-27)."""
    x = _f32c(x, "gdn")
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().dsic_gdn_nchw(_p(x), _p(beta_eff), _p(gamma_eff), _p(out), B, C, H * W,
                                         int(bool(inverse)), _stream()), "gdn")
    return out


def hyper_params(t_nhwc, w1s, b1s, w2s, b2s, w1n, b1n, w2n, b2n, M, min_nu, max_nu):
    """pool + MLP heads + exp/clamp -> (log_sigma, log_nu, sigma, nu), each [B,M]."""
    t = _f32c(t_nhwc, "hyper_params")
    B, H, W, N = t.shape
    outs = [torch.empty((B, M), dtype=torch.float32, device=t.device) for _ in range(4)]
    _lib.check(_lib.load().dsic_hyper_params(_p(t), _p(w1s), _p(b1s), _p(w2s), _p(b2s), _p(w1n), _p(b1n),
                                             _p(w2n), _p(b2n), _p(outs[0]), _p(outs[1]), _p(outs[2]),
                                             _p(outs[3]), B, H * W, N, M, float(min_nu), float(max_nu),
                                             _stream()), "hyper_params")
    return outs


def rate(y_nhwc, z_nhwc, sigma, nu, z_log_sigma, y_noisy=None, z_noisy=None):
    """round + Student-t/Gaussian bits + per-image sums.

    Returns dict(y_hat_nhwc, y_tilde, z_tilde, nll_y, nll_z (NCHW), sums [B,2] fp64).
    """
    y = _f32c(y_nhwc, "rate")
    z = _f32c(z_nhwc, "rate")
    B, Hy, Wy, M = y.shape
    _, Hz, Wz, N = z.shape
    dev = y.device
    y_hat = torch.empty_like(y)
    y_t = torch.empty((B, M, Hy, Wy), dtype=torch.float32, device=dev)
    nll_y = torch.empty_like(y_t)
    z_t = torch.empty((B, N, Hz, Wz), dtype=torch.float32, device=dev)
    nll_z = torch.empty_like(z_t)
    sums = torch.empty((B, 2), dtype=torch.float64, device=dev)
    work = torch.empty(_lib.load().dsic_rate_workspace_doubles(B), dtype=torch.float64, device=dev)
    per_element = 1 if sigma.dim() == 4 else 0          # [B,M,Hy,Wy] (spatial_params) vs [B,M]
    sigma = _f32c(sigma, "rate")
    nu = _f32c(nu, "rate")
    _lib.check(_lib.load().dsic_rate(_p(y), _p(z), _p(y_noisy), _p(z_noisy), _p(sigma), _p(nu),
                                     _p(z_log_sigma), _p(y_hat), _p(y_t), _p(z_t), _p(nll_y), _p(nll_z),
                                     _p(sums), _p(work), B, Hy * Wy, M, Hz * Wz, N, per_element, _stream()),
               "rate")
    return {"y_hat_nhwc": y_hat, "y_tilde": y_t, "z_tilde": z_t, "nll_y": nll_y, "nll_z": nll_z,
            "sums": sums}


def student_t_bits(x, sigma, nu):
    """StudentT.neg_log2_prob on NCHW x; sigma/nu full-shape or spatially constant."""
    x = _f32c(x, "student_t_bits")
    B, C, H, W = x.shape
    per_channel = 0
    if sigma.dim() == 4 and sigma.stride(2) == 0 and sigma.stride(3) == 0 \
            and nu.dim() == 4 and nu.stride(2) == 0 and nu.stride(3) == 0:
        sigma = sigma[:, :, 0, 0].expand(B, C)
        nu = nu[:, :, 0, 0].expand(B, C)
        per_channel = 1
    else:
        sigma = sigma.expand_as(x)
        nu = nu.expand_as(x)
    sigma = _f32c(sigma, "student_t_bits")
    nu = _f32c(nu, "student_t_bits")
    out = torch.empty_like(x)
    _lib.check(_lib.load().dsic_student_t_bits(_p(x), _p(sigma), _p(nu), _p(out), x.numel(), H * W,
                                               per_channel, _stream()), "student_t_bits")
    return out


def gaussian_bits(x, log_sigma):
    x = _f32c(x, "gaussian_bits")
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().dsic_gaussian_bits(_p(x), _p(_f32c(log_sigma, "gaussian_bits")), _p(out), B, C,
                                              H * W, _stream()), "gaussian_bits")
    return out


def sigma_nu_spatial(log_sigma_nhwc, log_nu_nhwc, min_nu, max_nu):
    """spatial_params head outputs (NHWC) -> sigma, nu NCHW [B,M,H,W] (model.py:49-51)."""
    ls = _f32c(log_sigma_nhwc, "sigma_nu_spatial")
    ln = _f32c(log_nu_nhwc, "sigma_nu_spatial")
    B, H, W, M = ls.shape
    sigma = torch.empty((B, M, H, W), dtype=torch.float32, device=ls.device)
    nu = torch.empty_like(sigma)
    _lib.check(_lib.load().dsic_sigma_nu_spatial(_p(ls), _p(ln), _p(sigma), _p(nu), B, H * W, M, float(min_nu),
                                                 float(max_nu), _stream()), "sigma_nu_spatial")
    return sigma, nu
