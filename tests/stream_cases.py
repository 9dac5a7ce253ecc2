"""One recipe per export of include/dsic_hip.h that takes a stream: everything a test needs to make that C-ABI call
on any stream, with two complete input sets A and B of the same shapes, and nothing that needs a GPU to build.

A recipe is a function of the loaded library (only its host-side size functions and predicates are asked) that
returns a Case:
  - inp():  an input buffer with its A and B contents (NumPy arrays of one shape and dtype).  `bound=(lo, hi)` marks
            an array of indices, lengths or ids that a kernel takes from device memory: lo <= v < hi is what the
            export's own argument check or header states, and it holds in A, in B and hence in any mixture of the
            two.  Where a mixture of two arrays would have to agree (a support with its table, a popcount with its
            plane) both sets hold the same values there, and the arrays beside them differ.
  - out():  an output buffer (dtype, elements); work(): a workspace, never an input and never judged.  Before every
            call, as part of `prepare`, a buffer the header makes the caller zero is zeroed (zero=True: histograms,
            counts, tickets, coder output) and every other output is refilled with FILL bytes, so that bytes a call
            leaves alone are the same bytes on every run; a workspace keeps what the last call left in it.
            inout=True on inp(): the call works in place (a blend canvas).
  - hostarr(): a host array the export reads before it returns (scales, band lists, warp matrices).
  - call(L, p, stream): the C-ABI call; p.<name> is a buffer's device address (an int), p.<host name> the ctypes
            array.  Returns the status.
  - reach(L): asserts that the shape reaches every launch the export can make.
  - restate(inputs) -> bytes: the CPU restatement of the outputs where the family has one at hand.

tests/test_stream_cases_cpu.py holds the recipes to the header; tests/test_gpu_stream_order.py runs them."""
import ctypes

import numpy as np

FILL = 0x5A                                    # float32 0x5A5A5A5A = 1.5e16, finite
U8, U16, I32, U32, I64, U64, F32, F64 = (np.dtype(t) for t in ("u1", "u2", "i4", "u4", "i8", "u8", "f4", "f8"))


class Case:
    def __init__(self, name, exports):
        self.name = name
        self.exports = [exports] if isinstance(exports, str) else list(exports)
        self.bufs = {}                         # name -> dict(kind, dtype, n, A, B, bound, zero, inout)
        self.host = {}
        self.call = None
        self.reach = None
        self.restate = None

    def inp(self, name, A, B, bound=None, inout=False):
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        assert A.shape == B.shape and A.dtype == B.dtype, (self.name, name)
        self.bufs[name] = dict(kind="in", dtype=A.dtype, n=A.size, A=A, B=B, bound=bound, zero=False, inout=inout)

    def same(self, name, A, bound=None):
        """an input that must agree with its neighbours in any mixture: one content for both sets"""
        self.inp(name, A, A, bound)

    def out(self, name, dtype, n, zero=False):
        self.bufs[name] = dict(kind="out", dtype=np.dtype(dtype), n=int(n), zero=zero, inout=False)

    def work(self, name, dtype, n, zero=False):
        self.bufs[name] = dict(kind="work", dtype=np.dtype(dtype), n=int(n), zero=zero, inout=False)

    def hostarr(self, name, ctype, values):
        self.host[name] = (ctype * len(values))(*values)

    def inputs(self, which):
        return {k: b[which] for k, b in self.bufs.items() if b["kind"] == "in"}

    def judged(self):
        """the buffers whose bytes are a result of the call"""
        return [k for k, b in self.bufs.items() if b["kind"] == "out" or b["inout"]]


class Ptrs:
    def __init__(self, addr, host):
        self.__dict__.update(addr)
        self.__dict__.update(host)
        self.null = None


def _rng(name, which):
    return np.random.default_rng([sum(name.encode()) * 7919 + len(name), 0 if which == "A" else 1])


def _f(rng, *shape, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, size=shape).astype(np.float32)


def _ab(c, name, make, **kw):
    """an input whose two sets come from one generator and two seeds"""
    A, B = make(_rng(c.name + name, "A")), make(_rng(c.name + name, "B"))
    assert A.tobytes() != B.tobytes(), (c.name, name)
    c.inp(name, A, B, **kw)
    return A, B


def _bf16_as(rng, n16, dtype):
    """n16 finite bf16 values (the upper halves of float32 values in (-1, 1)), seen as an array of `dtype`"""
    v = (rng.uniform(-1, 1, n16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return v.view(dtype)


RECIPES = []


def recipe(fn):
    RECIPES.append(fn)
    return fn


# ---- weight packing --------------------------------------------------------------------------------------------
def _pack_recipe(name, wshape, n_out, call, out_dtype=F32):
    def make(L):
        c = Case(name, "dsic_" + name)
        _ab(c, "w", lambda r: _f(r, *wshape))
        c.out("dst", out_dtype, n_out(L))
        c.call = lambda L, p, s: call(L, p, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_pack_recipe("pack_conv_weight", (8, 8, 3, 3), lambda L: L.dsic_packed_conv_weight_floats(8, 8, 3),
             lambda L, p, s: L.dsic_pack_conv_weight(p.w, p.dst, 8, 8, 3, s))
_pack_recipe("pack_convT_weight", (8, 8, 5, 5), lambda L: 25 * 1 * 32 * 8,
             lambda L, p, s: L.dsic_pack_convT_weight(p.w, p.dst, 8, 8, s))
_pack_recipe("pack_convT_image_weight", (16, 3, 5, 5), lambda L: L.dsic_convT_image_weight_floats(16),
             lambda L, p, s: L.dsic_pack_convT_image_weight(p.w, p.dst, 16, 3, s))
_pack_recipe("pack_wino_weight", (8, 32, 3, 3), lambda L: L.dsic_wino_weight_floats(8, 32),
             lambda L, p, s: L.dsic_pack_wino_weight(p.w, p.dst, 8, 32, s))
_pack_recipe("pack_wino_s2_weight", (8, 8, 5, 5), lambda L: L.dsic_wino_weight_floats(8, 32),
             lambda L, p, s: L.dsic_pack_wino_s2_weight(p.w, p.dst, 8, 8, s))
_pack_recipe("pack_wino_convT_weight", (32, 8, 5, 5), lambda L: 4 * L.dsic_wino_weight_floats(8, 32),
             lambda L, p, s: L.dsic_pack_wino_convT_weight(p.w, p.dst, 32, 8, s))


@recipe
def split_wino_weight_bf16(L):
    c = Case("split_wino_weight_bf16", "dsic_split_wino_weight_bf16")
    n = L.dsic_wino_weight_floats(8, 64)
    _ab(c, "u", lambda r: _f(r, n))
    c.out("dst", U8, L.dsic_wino_bf16_weight_bytes(8, 64))
    c.call = lambda L, p, s: L.dsic_split_wino_weight_bf16(p.u, p.dst, 8, 64, 1, s)
    return c


# ---- layout helpers --------------------------------------------------------------------------------------------
def _simple(name, ins, outs, call, exports=None, restate=None, zero=()):
    """ins: {name: fn(rng) -> array}; outs: {name: (dtype, n)}"""
    def make(L):
        c = Case(name, exports or "dsic_" + name)
        for k, v in ins.items():
            _ab(c, k, v)
        for k, (dt, n) in outs.items():
            c.out(k, dt, n, zero=k in zero)
        c.call = call
        c.restate = restate
        return c
    make.__name__ = name
    RECIPES.append(make)


_simple("image_to_nhwc8", {"x": lambda r: _f(r, 2, 3, 7, 37)}, {"dst": (F32, 2 * 7 * 37 * 8)},
        lambda L, p, s: L.dsic_image_to_nhwc8(p.x, p.dst, 2, 3, 7, 37, s))
_simple("nhwc_to_nchw", {"x": lambda r: _f(r, 2, 33, 65)}, {"dst": (F32, 2 * 33 * 65)},
        lambda L, p, s: L.dsic_nhwc_to_nchw(p.x, p.dst, 2, 3, 11, 65, s),
        restate=lambda i: i["x"].transpose(0, 2, 1).tobytes())
_simple("nchw_to_nhwc", {"x": lambda r: _f(r, 2, 65, 33)}, {"dst": (F32, 2 * 33 * 65)},
        lambda L, p, s: L.dsic_nchw_to_nhwc(p.x, p.dst, 2, 65, 3, 11, s),
        restate=lambda i: i["x"].transpose(0, 2, 1).tobytes())
_simple("reflect_pad_br", {"x": lambda r: _f(r, 3, 17, 33)}, {"dst": (F32, 3 * 32 * 48)},
        lambda L, p, s: L.dsic_reflect_pad_br(p.x, p.dst, 3, 17, 33, 15, 15, s),
        restate=lambda i: np.pad(i["x"], ((0, 0), (0, 15), (0, 15)), mode="reflect").tobytes())
_simple("normalize_bands", {"x": lambda r: _f(r, 3, 301, lo=0.0, hi=4000.0)},
        {"out01": (F32, 3 * 301), "u8": (U8, 3 * 301)},
        lambda L, p, s: L.dsic_normalize_bands(p.x, p.out01, p.u8, 3, 301, s))
_simple("image_u8hwc_to_f32nchw", {"x": lambda r: r.integers(0, 256, (2, 5, 13, 3), dtype=np.uint8)},
        {"dst": (F32, 2 * 3 * 5 * 13)},
        lambda L, p, s: L.dsic_image_u8hwc_to_f32nchw(p.x, p.dst, 2, 3, 5, 13, s),
        restate=lambda i: (i["x"].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)).tobytes())


# ---- convolutions ----------------------------------------------------------------------------------------------
def _act_inputs(c, Cout):
    _ab(c, "bias", lambda r: _f(r, Cout))
    _ab(c, "beta", lambda r: _f(r, Cout, lo=0.5, hi=1.5))
    _ab(c, "gamma", lambda r: _f(r, Cout, lo=0.0, hi=0.5))


@recipe
def conv2d_nhwc(L):
    c = Case("conv2d_nhwc", "dsic_conv2d_nhwc")
    B, H, W, Cin, Cout = 1, 9, 11, 8, 8
    _ab(c, "x", lambda r: _f(r, B, H, W, Cin))
    _ab(c, "w", lambda r: _f(r, L.dsic_packed_conv_weight_floats(Cout, Cin, 3)))
    _act_inputs(c, Cout)
    c.out("out", F32, B * H * W * Cout)
    c.call = lambda L, p, s: L.dsic_conv2d_nhwc(p.x, p.w, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 3, 1,
                                                1, s)
    return c


@recipe
def conv_transpose2d_nhwc(L):
    c = Case("conv_transpose2d_nhwc", "dsic_conv_transpose2d_nhwc")
    B, H, W, Cin, Cout = 1, 5, 7, 8, 8
    _ab(c, "x", lambda r: _f(r, B, H, W, Cin))
    _ab(c, "w", lambda r: _f(r, 25 * (Cin // 8) * 32 * 8))
    _act_inputs(c, Cout)
    c.out("out", F32, B * 4 * H * W * Cout)
    c.call = lambda L, p, s: L.dsic_conv_transpose2d_nhwc(p.x, p.w, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin,
                                                          Cout, 2, s)
    return c


@recipe
def conv_transpose2d_image(L):
    c = Case("conv_transpose2d_image", "dsic_conv_transpose2d_image")
    B, H, W, Cin, Cimg = 1, 5, 7, 16, 3
    n, n32 = L.dsic_convT_image_weight_floats(Cin), 9 * (Cin // 16) * 16 * 16
    _ab(c, "x", lambda r: _f(r, B, H, W, Cin))
    _ab(c, "w", lambda r: np.concatenate([_f(r, n32), _bf16_as(r, 2 * (n - n32), np.float32)]))
    _ab(c, "bias", lambda r: _f(r, Cimg))
    c.out("out", F32, B * Cimg * 4 * H * W)
    c.call = lambda L, p, s: L.dsic_conv_transpose2d_image(p.x, p.w, p.bias, p.out, B, H, W, Cin, Cimg, s)
    return c


def _first(name, u8):
    def make(L):
        c = Case(name, "dsic_" + name)
        B, Cimg, H, W, Cout = 1, 3, 9, 11, 8
        if u8:
            _ab(c, "x", lambda r: r.integers(0, 256, (B, H, W, Cimg), dtype=np.uint8))
        else:
            _ab(c, "x", lambda r: _f(r, B, Cimg, H, W, lo=0.0))
        _ab(c, "w", lambda r: _f(r, Cout, Cimg, 3, 3))
        _act_inputs(c, Cout)
        c.out("out", F32, B * H * W * Cout)
        fn = getattr(L, "dsic_" + name)
        c.call = lambda L, p, s: fn(p.x, p.w, p.bias, p.beta, p.gamma, p.out, B, Cimg, H, W, Cout, 1, 0, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_first("conv_first_nchw", False)
_first("conv_first_u8hwc", True)


def _wino(name, export, B, H, W, Cin, Cout, kind, nphase=1, reach=None):
    """kind: f32 / f32T / bf16 / splitk / bf16T / bf16L"""
    def make(L):
        c = Case(name, export)
        bf16 = kind in ("bf16", "splitk", "bf16T", "bf16L")
        _ab(c, "x", lambda r: _f(r, B, H, W, Cin))
        if bf16:
            nb = nphase * L.dsic_wino_bf16_weight_bytes(Cout, Cin)
            _ab(c, "u", lambda r: _bf16_as(r, nb // 2, np.uint16))
        else:
            _ab(c, "u", lambda r: _f(r, nphase * L.dsic_wino_weight_floats(Cout, Cin)))
        _act_inputs(c, Cout)
        up = 4 if nphase == 4 else 1
        n_out = B * H * W * up * Cout
        c.out("out", F32, n_out)
        c.work("ticket", I32, 4, zero=True)
        fn = getattr(L, export)
        if kind == "f32":
            c.call = lambda L, p, s: fn(p.x, p.u, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 1, 0, 0,
                                        p.ticket, s)
        elif kind in ("f32T", "bf16T"):
            c.call = lambda L, p, s: fn(p.x, p.u, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 2, p.ticket, s)
        elif kind == "bf16L":
            c.call = lambda L, p, s: fn(p.x, p.u, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 2, 0, 0,
                                        p.ticket, s)
        elif kind == "bf16":
            c.call = lambda L, p, s: fn(p.x, p.u, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 1, 0, 0, 0, 0,
                                        p.ticket, s)
        else:
            S = L.dsic_wino_bf16_ksplit(H, W, Cin)
            c.work("partials", F32, S * n_out)
            c.call = lambda L, p, s: fn(p.x, p.u, p.bias, p.beta, p.gamma, p.out, B, H, W, Cin, Cout, 1, 0, 0, 0, 0,
                                        S, p.partials, p.ticket, s)
        c.reach = reach
        return c
    make.__name__ = name
    RECIPES.append(make)


def _is_m64(H, W, Cin, nphase, want):
    def reach(L):
        assert L.dsic_wino_bf16_m64(H, W, Cin, nphase) == want
    return reach


def _is_split(L):
    assert L.dsic_wino_bf16_ksplit(16, 16, 128) > 1      # the partial sums and the launch that adds them


_wino("conv3x3_wino_nhwc", "dsic_conv3x3_wino_nhwc", 1, 9, 11, 32, 8, "f32")
_wino("conv_transpose2d_wino_nhwc", "dsic_conv_transpose2d_wino_nhwc", 1, 5, 7, 32, 8, "f32T", nphase=4)
_wino("conv3x3_wino_bf16_nhwc", "dsic_conv3x3_wino_bf16_nhwc", 1, 9, 11, 64, 8, "bf16",
      reach=_is_m64(9, 11, 64, 1, 0))
_wino("conv3x3_wino_bf16_nhwc_m64", "dsic_conv3x3_wino_bf16_nhwc", 1, 32, 32, 64, 16, "bf16",
      reach=_is_m64(32, 32, 64, 1, 1))
_wino("conv3x3_wino_bf16_splitk_nhwc", "dsic_conv3x3_wino_bf16_splitk_nhwc", 1, 16, 16, 128, 128, "splitk",
      reach=_is_split)
_wino("conv_transpose2d_wino_bf16_nhwc", "dsic_conv_transpose2d_wino_bf16_nhwc", 1, 5, 7, 64, 8, "bf16T", nphase=4,
      reach=_is_m64(5, 7, 64, 4, 0))
_wino("conv_transpose2d_wino_bf16_nhwc_m64", "dsic_conv_transpose2d_wino_bf16_nhwc", 1, 16, 16, 64, 16, "bf16T",
      nphase=4, reach=_is_m64(16, 16, 64, 4, 1))
_wino("conv_transpose2d_wino_bf16_layout", "dsic_conv_transpose2d_wino_bf16_layout", 1, 5, 7, 64, 8, "bf16L",
      nphase=4)


# ---- hyper-synthesis heads, quantisation, rate -----------------------------------------------------------------
@recipe
def hyper_params(L):
    c = Case("hyper_params", "dsic_hyper_params")
    B, HW, N, M = 2, 6, 128, 192
    _ab(c, "t", lambda r: _f(r, B, HW, N, lo=0.0))
    for h in ("s", "n"):
        _ab(c, "w1" + h, lambda r: _f(r, N, N, lo=-0.1, hi=0.1))
        _ab(c, "b1" + h, lambda r: _f(r, N))
        _ab(c, "w2" + h, lambda r: _f(r, N, M, lo=-0.1, hi=0.1))
        _ab(c, "b2" + h, lambda r: _f(r, M))
    for o in ("ls", "ln", "sg", "nu"):
        c.out(o, F32, B * M)
    c.call = lambda L, p, s: L.dsic_hyper_params(p.t, p.w1s, p.b1s, p.w2s, p.b2s, p.w1n, p.b1n, p.w2n, p.b2n, p.ls,
                                                 p.ln, p.sg, p.nu, B, HW, N, M, 2.0, 100.0, s)
    return c


@recipe
def rate(L):
    c = Case("rate", "dsic_rate")
    B, HWy, M, HWz, N = 2, 35, 16, 6, 8
    _ab(c, "y", lambda r: _f(r, B, HWy, M, lo=-9.0, hi=9.0))
    _ab(c, "z", lambda r: _f(r, B, HWz, N, lo=-5.0, hi=5.0))
    _ab(c, "sigma", lambda r: _f(r, B, M, lo=0.5, hi=4.0))
    _ab(c, "nu", lambda r: _f(r, B, M, lo=2.0, hi=40.0))
    _ab(c, "zls", lambda r: _f(r, N))
    c.out("y_hat", F32, B * HWy * M)
    c.out("y_tilde", F32, B * HWy * M)
    c.out("z_tilde", F32, B * HWz * N)
    c.out("nll_y", F32, B * HWy * M)
    c.out("nll_z", F32, B * HWz * N)
    c.out("sums", F64, 2 * B)
    c.work("work", F64, L.dsic_rate_workspace_doubles(B))
    c.call = lambda L, p, s: L.dsic_rate(p.y, p.z, None, None, p.sigma, p.nu, p.zls, p.y_hat, p.y_tilde, p.z_tilde,
                                         p.nll_y, p.nll_z, p.sums, p.work, B, HWy, M, HWz, N, 0, s)
    return c


_simple("sigma_nu_spatial", {"ls": lambda r: _f(r, 2, 35, 16), "ln": lambda r: _f(r, 2, 35, 16, lo=0.0, hi=4.0)},
        {"sg": (F32, 2 * 35 * 16), "nu": (F32, 2 * 35 * 16)},
        lambda L, p, s: L.dsic_sigma_nu_spatial(p.ls, p.ln, p.sg, p.nu, 2, 35, 16, 2.0, 100.0, s))
_simple("student_t_bits", {"x": lambda r: np.rint(_f(r, 2 * 16 * 35, lo=-9.0, hi=9.0)),
                           "sigma": lambda r: _f(r, 2 * 16, lo=0.5, hi=4.0),
                           "nu": lambda r: _f(r, 2 * 16, lo=2.0, hi=40.0)}, {"out": (F32, 2 * 16 * 35)},
        lambda L, p, s: L.dsic_student_t_bits(p.x, p.sigma, p.nu, p.out, 2 * 16 * 35, 35, 1, s))
_simple("gaussian_bits", {"x": lambda r: np.rint(_f(r, 2, 8, 35, lo=-5.0, hi=5.0)), "ls": lambda r: _f(r, 8)},
        {"out": (F32, 2 * 8 * 35)}, lambda L, p, s: L.dsic_gaussian_bits(p.x, p.ls, p.out, 2, 8, 35, s))
_simple("round", {"x": lambda r: _f(r, 1031, lo=-9.0, hi=9.0)}, {"out": (F32, 1031)},
        lambda L, p, s: L.dsic_round(p.x, p.out, 1031, s), restate=lambda i: np.rint(i["x"]).tobytes())
_simple("gdn_nchw", {"x": lambda r: _f(r, 2, 8, 35), "beta": lambda r: _f(r, 8, lo=0.5, hi=1.5),
                     "gamma": lambda r: _f(r, 8, lo=0.0, hi=0.5)}, {"out": (F32, 2 * 8 * 35)},
        lambda L, p, s: L.dsic_gdn_nchw(p.x, p.beta, p.gamma, p.out, 2, 8, 35, 0, s))


# ---- distortion metrics ----------------------------------------------------------------------------------------
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _ssim(name, export, H, W, pool, reach=None):
    def make(L):
        c = Case(name, export)
        planes = 3
        _ab(c, "X", lambda r: _f(r, planes, H, W, lo=-0.1, hi=1.1))
        _ab(c, "Y", lambda r: _f(r, planes, H, W, lo=0.0))
        c.work("partial", F64, L.dsic_ssim_partial_doubles(planes, H, W))
        c.out("means", F64, 2 * planes)
        if pool:
            Hn, Wn = (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1
            c.out("Xn", F32, planes * Hn * Wn)
            c.out("Yn", F32, planes * Hn * Wn)
            c.call = lambda L, p, s: L.dsic_ssim_level_pool(p.X, p.Y, p.partial, p.means, p.Xn, p.Yn, planes, H, W,
                                                            C1, C2, 1, s)
        else:
            c.call = lambda L, p, s: L.dsic_ssim_level(p.X, p.Y, p.partial, p.means, planes, H, W, C1, C2, 1, s)
        c.reach = reach
        return c
    make.__name__ = name
    RECIPES.append(make)


def _fused(H, W, want):
    def reach(L):
        assert L.dsic_ssim_level_pool_fused(H, W) == want
    return reach


_ssim("ssim_level", "dsic_ssim_level", 40, 68, False)                        # level, then reduce
_ssim("ssim_level_pool_fused", "dsic_ssim_level_pool", 40, 68, True, _fused(40, 68, 1))
_ssim("ssim_level_pool_unfused", "dsic_ssim_level_pool", 41, 67, True, _fused(41, 67, 0))   # level + reduce + 2 pools
_simple("avgpool2", {"x": lambda r: _f(r, 3, 41, 67, lo=-0.1, hi=1.1)}, {"dst": (F32, 3 * 21 * 34)},
        lambda L, p, s: L.dsic_avgpool2(p.x, p.dst, 3, 41, 67, 1, s))
_simple("msssim_finalize", {"means": lambda r: r.uniform(0.2, 1.0, (5, 6, 2)),
                            "weights": lambda r: _f(r, 5, lo=0.1, hi=0.4)}, {"out": (F32, 2)},
        lambda L, p, s: L.dsic_msssim_finalize(p.means, p.weights, p.out, 5, 2, 3, 1, s))
_simple("sqerr_per_image", {"a": lambda r: _f(r, 2, 3 * 40 * 68, lo=-0.1, hi=1.1),
                            "b": lambda r: _f(r, 2, 3 * 40 * 68, lo=0.0)}, {"out": (F64, 2)},
        lambda L, p, s: L.dsic_sqerr_per_image(p.a, p.b, p.out, 2, 3 * 40 * 68, 1, s))


# ---- entropy coding --------------------------------------------------------------------------------------------
# One support for both sets (a table is only a table under its own support); symbols, parameters and tables differ.
CODER = dict(B=2, M=8, Hy=13, Wy=11, N=3, Hz=1, Wz=5, Lmax=64, meta=(-24, 49, -12, 25))


def _cap(n):
    return (2 * n + 16 + 3) // 4 * 4


def _coder_meta():
    return np.tile(np.array(CODER["meta"], dtype=np.int32), (CODER["B"], 1))


def _host_tables(L, rng, rows, student, smin, Lsup):
    Lmax = CODER["Lmax"]
    tab = np.zeros((rows, Lmax), dtype=np.uint16)
    row = (ctypes.c_uint16 * Lsup)()
    for i in range(rows):
        sigma, nu = float(rng.uniform(0.8, 6.0)), float(rng.uniform(2.0, 50.0))
        assert L.dsic_host_cdf_table(student, sigma, nu, smin, Lsup, row, None) == 0
        tab[i, :Lsup] = np.frombuffer(row, dtype=np.uint16)
    return tab


def _coder_inputs(c, L):
    k = CODER
    ymin, Ly, zmin, Lz = k["meta"]
    _ab(c, "y", lambda r: np.rint(r.standard_t(3.0, (k["B"], k["M"], k["Hy"] * k["Wy"])) * 3).clip(-20, 20)
        .astype(np.float32))
    _ab(c, "z", lambda r: np.rint(r.normal(size=(k["B"], k["N"], k["Hz"] * k["Wz"])) * 3).clip(-10, 10)
        .astype(np.float32))
    c.same("meta", _coder_meta())
    _ab(c, "tab_y", lambda r: _host_tables(L, r, k["B"] * k["M"], 1, ymin, Ly))
    _ab(c, "tab_z", lambda r: _host_tables(L, r, k["B"] * k["N"], 0, zmin, Lz))


def _slices(segs):
    """the place step's slicing restated for short strings: a slice is 8 groups of 64 symbols"""
    def reach(L):
        k = CODER
        n = k["M"] * k["Hy"] * k["Wy"] // max(segs, 1)
        assert -(-(-(-n // 64)) // 8) > 1          # a y string (or segment) is placed in more than one slice
    return reach


@recipe
def latent_support(L):
    c = Case("latent_support", "dsic_latent_support")
    k = CODER
    ny, nz = k["M"] * k["Hy"] * k["Wy"], k["N"] * k["Hz"] * k["Wz"]
    _ab(c, "y", lambda r: np.rint(r.standard_t(3.0, (k["B"], ny)) * 3).clip(-40, 40).astype(np.float32))
    _ab(c, "z", lambda r: np.rint(r.normal(size=(k["B"], nz)) * 3).astype(np.float32))
    c.out("meta", I32, 4 * k["B"])
    c.call = lambda L, p, s: L.dsic_latent_support(p.y, p.z, p.meta, k["B"], ny, nz, 10, s)

    def restate(i):
        rows = []
        for b in range(k["B"]):
            row = []
            for v in (i["y"][b], i["z"][b]):
                lo, hi = int(np.floor(v.min())), int(np.ceil(v.max()))
                row += [lo - 10, hi - lo + 21]
            rows.append(row)
        return np.array(rows, dtype=np.int32).tobytes()
    c.restate = restate
    return c


def _meta_sets(rng, B, Lmax):
    m = np.stack([rng.integers(-30, 1, B), rng.integers(20, Lmax + 1, B), rng.integers(-15, 1, B),
                  rng.integers(10, Lmax + 1, B)], 1).astype(np.int32)
    return m


@recipe
def cdf_tables_gauss(L):
    c = Case("cdf_tables_gauss", "dsic_cdf_tables_gauss")
    B, N, Lmax = 3, 6, 64
    _ab(c, "sigma", lambda r: _f(r, N, lo=0.5, hi=6.0))
    _ab(c, "meta", lambda r: _meta_sets(r, B, Lmax))          # the export checks every L against Lmax itself
    c.out("tables", U16, B * N * Lmax)
    c.out("err", I32, 1, zero=True)
    c.call = lambda L, p, s: L.dsic_cdf_tables_gauss(p.sigma, p.meta, p.tables, B, N, Lmax, p.err, s)
    return c


@recipe
def cdf_tables_student(L):
    c = Case("cdf_tables_student", "dsic_cdf_tables_student")
    B, M, Lmax = 3, 5, 64
    _ab(c, "sigma", lambda r: _f(r, B, M, lo=0.5, hi=6.0))
    _ab(c, "nu", lambda r: _f(r, B, M, lo=2.0, hi=50.0))
    _ab(c, "meta", lambda r: _meta_sets(r, B, Lmax))
    c.out("tables", U16, B * M * Lmax)
    c.out("err", I32, 1, zero=True)
    c.call = lambda L, p, s: L.dsic_cdf_tables_student(p.sigma, p.nu, p.meta, p.tables, B, M, Lmax, p.err, s)
    return c


def _encode(name, segs):
    def make(L):
        c = Case(name, "dsic_" + name)
        k = CODER
        B, M, HWy, N, HWz, Lmax = k["B"], k["M"], k["Hy"] * k["Wy"], k["N"], k["Hz"] * k["Wz"], k["Lmax"]
        _coder_inputs(c, L)
        cap_z = _cap(N * HWz)
        cap_y = _cap(M * HWy // max(segs, 1))
        K = max(segs, 1)
        c.out("out", U8, B * (cap_z + K * cap_y), zero=True)
        c.out("lengths", I32, B * (1 + K), zero=True)
        c.out("err", I32, 1, zero=True)
        if name == "range_encode":
            c.call = lambda L, p, s: L.dsic_range_encode(p.y, p.z, p.meta, p.tab_y, p.tab_z, Lmax, B, M, HWy, N, HWz,
                                                         p.out, cap_y, cap_z, p.lengths, p.err, 1, 0, s)
        elif name == "range_encode_ws":
            nb = L.dsic_range_encode_workspace_size(B, M, HWy, N, HWz)
            c.work("ws", U8, nb)
            c.call = lambda L, p, s: L.dsic_range_encode_ws(p.y, p.z, p.meta, p.tab_y, p.tab_z, Lmax, B, M, HWy, N,
                                                            HWz, p.out, cap_y, cap_z, p.lengths, p.err, 0, p.ws, nb,
                                                            s)
            c.reach = _slices(segs)
        else:
            nb = L.dsic_range_encode_seg_workspace_size(B, M, HWy, N, HWz, segs)
            c.work("ws", U8, nb)
            c.call = lambda L, p, s: L.dsic_range_encode_seg_ws(p.y, p.z, p.meta, p.tab_y, p.tab_z, Lmax, B, M, HWy,
                                                                N, HWz, p.out, cap_y, cap_z, p.lengths, p.err, 0,
                                                                segs, p.ws, nb, s)
            c.reach = _slices(segs)
        return c
    make.__name__ = name
    RECIPES.append(make)


_encode("range_encode", 0)
_encode("range_encode_ws", 0)
_encode("range_encode_seg_ws", 2)


def _decode(name, segs):
    def make(L):
        c = Case(name, "dsic_" + name)
        k = CODER
        B, M, HW, Lmax = k["B"], k["M"], k["Hy"] * k["Wy"], k["Lmax"]
        ymin, Ly, _, _ = k["meta"]
        stride = 1024
        # any bytes decode to symbols inside the support, so the strings are plain random bytes
        _ab(c, "bytes", lambda r: r.integers(0, 256, B * stride, dtype=np.uint8))
        _ab(c, "lengths", lambda r: r.integers(600, stride + 1, (B, 2)).astype(np.int32), bound=(0, stride + 1))
        c.same("meta", _coder_meta())
        _ab(c, "tables", lambda r: _host_tables(L, r, B * M, 1, ymin, Ly))
        c.out("out", F32, B * M * HW)
        c.out("err", I32, 1, zero=True)
        if segs:
            _ab(c, "seg", lambda r: r.integers(100, 300, (B, segs)).astype(np.int32), bound=(0, stride + 1))
            c.call = lambda L, p, s: L.dsic_range_decode_seg(p.bytes, stride, p.lengths, 2, 1, p.seg, segs, p.meta, 0,
                                                             p.tables, Lmax, B, M, HW, 0, p.out, p.err, s)
        else:
            c.call = lambda L, p, s: L.dsic_range_decode(p.bytes, stride, p.lengths, 2, 1, p.meta, 0, p.tables, Lmax,
                                                         B, M, HW, 0, p.out, p.err, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_decode("range_decode", 0)
_decode("range_decode_seg", 2)


# ---- image codec: tile movers, containers ----------------------------------------------------------------------
IH, IW, TILE, OV = 40, 70, 32, 16                # 2 x 3 tiles of 32 (the last of each axis shifted inward); 2 x 4 with overlap 16
N_TILES, N_TILES_OV = 6, 8
WIN = (1, 1, IH - 2, IW - 3)                     # wy0, wx0, wh, ww


def _img(dtype, C):
    hi = 256 if dtype == np.uint8 else 65536
    return lambda r: r.integers(0, hi, (IH, IW, C), dtype=dtype)


def _tiles(n, C, lo=-0.25, hi=1.25):
    return lambda r: _f(r, n, C, TILE, TILE, lo=lo, hi=hi)


def _ids(c, n):
    c.inp("ids", np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy(), bound=(0, n))


def _lohi(c, C):
    c.hostarr("lohi", ctypes.c_uint32, [100, 60000, 0, 65535, 5000, 5000, 7, 40000][:2 * C])


def _gather(kind, ov):
    name = f"tile_gather_{kind}" + ("_ov" if ov else "")

    def make(L):
        c = Case(name, "dsic_" + name)
        C = 3
        n = N_TILES_OV if ov else N_TILES
        if kind == "f32":
            _ab(c, "img", lambda r: _f(r, C, IH, IW, lo=0.0))
        else:
            _ab(c, "img", _img(np.uint8 if kind == "u8" else np.uint16, C))
        c.out("tiles", U8 if kind == "u8" else F32, n * C * TILE * TILE)
        fn = getattr(L, "dsic_" + name)
        extra = (OV,) if ov else ()
        if kind == "u16":
            _lohi(c, C)
            c.call = lambda L, p, s: fn(p.img, p.tiles, IH, IW, C, TILE, TILE, *extra, p.lohi, 0, n, s)
        else:
            c.call = lambda L, p, s: fn(p.img, p.tiles, IH, IW, C, TILE, TILE, *extra, 0, n, s)
        if not ov and kind != "u16":
            import codec_ref as R
            c.restate = lambda i: (R.gather_u8 if kind == "u8" else R.gather_f32)(i["img"], TILE, TILE).tobytes()
        return c
    make.__name__ = name
    RECIPES.append(make)


for _k in ("u8", "f32", "u16"):
    _gather(_k, False)
    _gather(_k, True)


def _stitch(name, kind, window, res=False):
    def make(L):
        c = Case(name, "dsic_" + name)
        C = 3
        odt = {"u8": U8, "u16": U16, "f32": F32}[kind]
        _ab(c, "tiles", _tiles(N_TILES, C))
        fn = getattr(L, "dsic_" + name)
        if not window:
            c.out("img", odt, C * IH * IW)
            c.call = lambda L, p, s: fn(p.tiles, p.img, IH, IW, C, TILE, TILE, 0, N_TILES, s)
            return c
        _ids(c, N_TILES)
        wy, wx, wh, ww = WIN
        c.out("img", odt, C * wh * ww)
        geo = (IH, IW, C, TILE, TILE, wy, wx, wh, ww)
        if kind == "u16":
            _lohi(c, C)
        if res:
            tau = 2 if kind == "u8" else 40
            _ab(c, "q", lambda r: np.rint(_f(r, N_TILES, C, TILE, TILE, lo=-20.0, hi=20.0)))
            if kind == "u16":
                c.call = lambda L, p, s: fn(p.tiles, p.q, tau, p.ids, N_TILES, p.img, *geo, p.lohi, s)
            else:
                c.call = lambda L, p, s: fn(p.tiles, p.q, tau, p.ids, N_TILES, p.img, *geo, s)
        elif kind == "u16":
            c.call = lambda L, p, s: fn(p.tiles, p.ids, N_TILES, p.img, *geo, p.lohi, s)
        else:
            c.call = lambda L, p, s: fn(p.tiles, p.ids, N_TILES, p.img, *geo, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_stitch("tile_stitch_f32", "f32", False)
_stitch("tile_stitch_u8", "u8", False)
_stitch("tile_stitch_window_f32", "f32", True)
_stitch("tile_stitch_window_u8", "u8", True)
_stitch("tile_stitch_window_u16", "u16", True)
_stitch("tile_stitch_window_u8_res", "u8", True, res=True)
_stitch("tile_stitch_window_u16_res", "u16", True, res=True)

CAP_Z, CAP_Y, TAG = 8, 5120, 0xDEADBEEF          # strings over 4 KiB: copied by more than one workgroup part each
SHAPE = (4, 6, 5, 1, 2)                          # Hy, Wy, Nz, Hz, Wz


def _strings(c, B, K, same_lengths=False):
    rows = _ab(c, "rows", lambda r: r.integers(1, 256, (B, CAP_Z + K * CAP_Y), dtype=np.uint8))

    def lengths(r):
        a = np.concatenate([r.integers(0, CAP_Z + 1, (B, 1)), r.integers(4097, CAP_Y + 1, (B, K))], 1)
        return a.astype(np.int32)
    if same_lengths:
        ln = lengths(_rng(c.name, "A"))
        c.same("lengths", ln, bound=(0, CAP_Y + 1))
        ln = (ln, ln)
    else:
        ln = _ab(c, "lengths", lengths, bound=(0, CAP_Y + 1))
    meta = _ab(c, "meta", lambda r: np.stack([r.integers(-40, 1, B), r.integers(1, 90, B), r.integers(-9, 1, B),
                                              r.integers(1, 20, B)], 1).astype(np.int32))
    return rows, ln, meta


def _parts(L):
    assert CAP_Y > 4096


@recipe
def container_pack(L):
    c = Case("container_pack", "dsic_container_pack")
    B = 3
    _strings(c, B, 1)
    c.work("ws", I64, 2 * B + 3)
    c.out("out", U8, 38 + 24 * B + B * (CAP_Z + CAP_Y))
    c.call = lambda L, p, s: L.dsic_container_pack(p.rows, CAP_Z, CAP_Y, p.lengths, p.meta, None, B, TAG, 16, *SHAPE,
                                                   p.ws, p.out, s)
    c.reach = _parts

    def restate(i):
        import codec_ref as R
        return R.pack_container(i["rows"], i["lengths"], i["meta"], TAG, 16, *SHAPE, CAP_Z, CAP_Y, 1)[0]
    c.restate = restate
    return c


@recipe
def container_pack_seg(L):
    c = Case("container_pack_seg", "dsic_container_pack_seg")
    B, K = 3, 2
    _strings(c, B, K)
    c.work("ws", I64, B * (1 + K) + 3)
    c.out("out", U8, 42 + (24 + 4 * K) * B + B * (CAP_Z + K * CAP_Y))
    c.call = lambda L, p, s: L.dsic_container_pack_seg(p.rows, CAP_Z, CAP_Y, K, p.lengths, p.meta, None, B, TAG, 32,
                                                       *SHAPE, p.ws, p.out, s)
    c.reach = _parts
    return c


def _blobs(c, B):
    """two DSIC2 containers of one size: the same lengths (the scatter takes them from the blob), other bytes"""
    import codec_ref as R
    t = Case(c.name + "_strings", [])
    rows, ln, meta = _strings(t, B, 1, same_lengths=True)
    out = []
    for w in (0, 1):
        blob, total, offsets = R.pack_container(rows[w], ln[w], meta[w], TAG, 16, *SHAPE, CAP_Z, CAP_Y, 1)
        a = np.full(R.ceil16(total) + 16, 0x99, dtype=np.uint8)
        a[:total] = np.frombuffer(bytes(blob), dtype=np.uint8)
        out.append(a)
    c.inp("blob", out[0], out[1])
    return total, offsets, ln[0]


@recipe
def container_scatter(L):
    c = Case("container_scatter", "dsic_container_scatter")
    B = 3
    total, _, _ = _blobs(c, B)
    c.out("z", U8, B * CAP_Z)
    c.out("y", U8, B * CAP_Y)
    c.out("lengths", I32, 2 * B)
    c.out("meta", I32, 4 * B)
    c.work("ws", I64, 2 * B + 3)
    c.call = lambda L, p, s: L.dsic_container_scatter(p.blob, total, B, CAP_Y, p.z, CAP_Z, p.y, CAP_Y, p.lengths,
                                                      p.meta, p.ws, s)
    c.reach = _parts
    return c


@recipe
def strings_scatter_select(L):
    c = Case("strings_scatter_select", "dsic_strings_scatter_select")
    B = 3
    total, offsets, ln = _blobs(c, B)
    base = 38 + 24 * B
    d = np.array([[base + offsets[2 * b], ln[b, 0], base + offsets[2 * b + 1], ln[b, 1]] for b in range(B)],
                 dtype=np.int64)
    c.inp("desc", d, d[::-1].copy(), bound=(0, total))        # offsets and lengths inside the blob, either order
    c.out("z", U8, B * CAP_Z)
    c.out("y", U8, B * CAP_Y)
    c.out("lengths", I32, 2 * B)
    c.call = lambda L, p, s: L.dsic_strings_scatter_select(p.blob, total, p.desc, B, CAP_Y, p.z, CAP_Z, p.y, CAP_Y,
                                                           p.lengths, s)
    return c


@recipe
def tile_blend_window_f32(L):
    c = Case("tile_blend_window_f32", "dsic_tile_blend_window_f32")
    C = 3
    _ab(c, "tiles", _tiles(N_TILES_OV, C))
    c.same("ids", np.arange(N_TILES_OV, dtype=np.int32), bound=(0, N_TILES_OV))     # strictly ascending
    c.out("canvas", F32, C * IH * IW, zero=True)
    c.call = lambda L, p, s: L.dsic_tile_blend_window_f32(p.tiles, p.ids, N_TILES_OV, p.canvas, IH, IW, C, TILE, TILE,
                                                          OV, 0, 0, IH, IW, s)
    return c


def _canvas(r):
    a = _f(r, 3, IH, IW, lo=0.0, hi=1.0)
    a.ravel()[::17] = np.nextafter(np.float32(1.0), np.float32(2.0))
    return a


@recipe
def tile_blend_finish_f32(L):
    c = Case("tile_blend_finish_f32", "dsic_tile_blend_finish_f32")
    _ab(c, "canvas", _canvas, inout=True)
    c.call = lambda L, p, s: L.dsic_tile_blend_finish_f32(p.canvas, 3, IH, IW, s)
    c.restate = lambda i: np.minimum(i["canvas"], np.float32(1.0)).tobytes()
    return c


def _finish(kind):
    name = "tile_blend_finish_" + kind

    def make(L):
        c = Case(name, "dsic_" + name)
        _ab(c, "canvas", _canvas)
        c.out("out", U8 if kind == "u8" else U16, 3 * IH * IW)
        if kind == "u16":
            _lohi(c, 3)
            c.call = lambda L, p, s: L.dsic_tile_blend_finish_u16(p.canvas, p.out, 3, IH, IW, p.lohi, s)
        else:
            c.call = lambda L, p, s: L.dsic_tile_blend_finish_u8(p.canvas, p.out, 3, IH, IW, s)
            c.restate = lambda i: (np.minimum(i["canvas"], np.float32(1.0)) * np.float32(255.0)).astype(np.uint8) \
                .transpose(1, 2, 0).tobytes()
        return c
    make.__name__ = name
    RECIPES.append(make)


_finish("u8")
_finish("u16")


# ---- residual layers -------------------------------------------------------------------------------------------
RN, RC, TAU = 2, 3, 2
RQ = (255 + TAU) // (2 * TAU + 1)
RLMAX = (2 * RQ + 1 + 7) // 8 * 8
RCAP_Z, RCAP_SEG = 8, 64


def _quantize_u8(RC):
    name = "residual_quantize_u8" + ("" if RC == 3 else "_c4")

    def make(L):
        return _quantize_u8_case(name, RC)
    make.__name__ = name
    RECIPES.append(make)


def _quantize_u8_case(name, RC):
    c = Case(name, "dsic_residual_quantize_u8")
    _ab(c, "tiles", lambda r: r.integers(0, 256, (RN, TILE, TILE, RC), dtype=np.uint8))
    _ab(c, "x_hat", _tiles(RN, RC, lo=-0.1, hi=1.1))
    c.inp("own", np.array([[0, 32, 0, 32], [0, 20, 3, 32]], dtype=np.int32),
          np.array([[1, 32, 0, 30], [0, 32, 0, 32]], dtype=np.int32), bound=(0, TILE + 1))
    c.out("q", F32, RN * RC * TILE * TILE)
    c.out("hist", I32, RN * RC * 512, zero=True)
    c.call = lambda L, p, s: L.dsic_residual_quantize_u8(p.tiles, p.x_hat, p.own, RN, RC, TILE, TILE, TAU, p.q,
                                                         p.hist, s)
    return c


_quantize_u8(3)
_quantize_u8(4)


def _hist(Q, C):
    def make(r):
        h = np.zeros((RN, C, 512), dtype=np.int32)
        for t in range(RN):
            for ch in range(C):
                q = np.rint(r.normal(size=TILE * TILE) * 6).clip(-Q, Q).astype(np.int64)
                h[t, ch] = np.bincount(q + Q, minlength=512)
        return h
    return make


@recipe
def residual_tables(L):
    c = Case("residual_tables", "dsic_residual_tables")
    _ab(c, "hist", _hist(RQ, RC))
    c.out("meta", I32, 4 * RN)
    c.out("compact", U16, RN * RC * RLMAX)
    c.out("coder", U16, RN * RC * 16 * RLMAX)
    c.call = lambda L, p, s: L.dsic_residual_tables(p.hist, RN, RC, TILE, TILE, TAU, RLMAX, p.meta, p.compact,
                                                    p.coder, s)
    return c


@recipe
def residual_tables_u16(L):
    c = Case("residual_tables_u16", "dsic_residual_tables_u16")
    _ab(c, "hist", _hist(255, RC))
    c.out("meta", I32, 4 * RN)
    c.out("compact", U16, RN * RC * 512)
    c.out("coder", U16, RN * RC * 16 * 512)
    c.call = lambda L, p, s: L.dsic_residual_tables_u16(p.hist, RN, RC, TILE, TILE, p.meta, p.compact, p.coder, s)
    return c


def _res_strings(c, Lmax):
    _ab(c, "bytes", lambda r: r.integers(1, 256, (RN, RCAP_Z + 16 * RCAP_SEG), dtype=np.uint8))
    _ab(c, "lengths", lambda r: np.concatenate([r.integers(0, RCAP_Z + 1, (RN, 1)),
                                                r.integers(0, RCAP_SEG + 1, (RN, 16))], 1).astype(np.int32),
        bound=(0, RCAP_SEG + 1))
    c.same("meta", np.array([[-9, 20, 0, 1], [-30, 57, 0, 1]], dtype=np.int32), bound=(-255, Lmax + 1))
    _ab(c, "compact", lambda r: r.integers(0, 65536, (RN, RC, Lmax)).astype(np.uint16))


@recipe
def residual_pack(L):
    c = Case("residual_pack", "dsic_residual_pack")
    _res_strings(c, RLMAX)
    c.work("ws", I64, (RC + 16) * RN + 3)
    c.out("out", U8, 30 + 76 * RN + RN * (2 * RC * RLMAX + 16 * RCAP_SEG))
    c.call = lambda L, p, s: L.dsic_residual_pack(p.bytes, RCAP_Z, RCAP_SEG, p.lengths, p.meta, p.compact, None, RN,
                                                  RC, TILE, TILE, TAU, RLMAX, p.ws, p.out, s)
    return c


PLANE_WORDS = RC * TILE * TILE // 64


@recipe
def residual_pack_u16(L):
    c = Case("residual_pack_u16", "dsic_residual_pack_u16")
    _res_strings(c, 512)
    c.same("k", np.array([3, 9], dtype=np.int32), bound=(0, 10))
    _ab(c, "planes", lambda r: r.integers(0, 2 ** 63, (RN, 9, PLANE_WORDS)).astype(np.uint64))
    c.work("ws", I64, (RC + 17) * RN + 3)
    c.out("out", U8, 30 + 80 * RN + RN * (2 * RC * 512 + 9 * RC * TILE * TILE // 8 + 16 * RCAP_SEG))
    c.call = lambda L, p, s: L.dsic_residual_pack_u16(p.bytes, RCAP_Z, RCAP_SEG, p.lengths, p.meta, p.k, p.compact,
                                                      p.planes, None, RN, RC, TILE, TILE, 40, p.ws, p.out, s)
    return c


@recipe
def residual_quantize_u16(L):
    c = Case("residual_quantize_u16", "dsic_residual_quantize_u16")
    _ab(c, "img", _img(np.uint16, RC))
    _ab(c, "x_hat", _tiles(N_TILES, RC, lo=-0.1, hi=1.1))
    _lohi(c, RC)
    c.out("q", I32, N_TILES * RC * TILE * TILE)
    c.out("maxabs", I32, N_TILES, zero=True)
    c.call = lambda L, p, s: L.dsic_residual_quantize_u16(p.img, p.x_hat, IH, IW, RC, TILE, TILE, p.lohi, 40, 0,
                                                          N_TILES, p.q, p.maxabs, s)
    return c


@recipe
def residual_split_u16(L):
    c = Case("residual_split_u16", "dsic_residual_split_u16")
    q = _ab(c, "q", lambda r: r.integers(-700, 701, (RN, RC, TILE, TILE)).astype(np.int32) * np.int32([[[[1]]], [[[3]]]]))
    c.inp("maxabs", *[np.abs(a).reshape(RN, -1).max(1).astype(np.int32) for a in q])
    c.out("hi", F32, RN * RC * TILE * TILE)
    c.out("hist", I32, RN * RC * 512, zero=True)
    c.out("k", I32, RN)
    c.out("planes", U64, RN * 9 * PLANE_WORDS)
    c.call = lambda L, p, s: L.dsic_residual_split_u16(p.q, p.maxabs, RN, RC, TILE, TILE, p.hi, p.hist, p.k, p.planes,
                                                       s)
    return c


@recipe
def residual_join_u16(L):
    c = Case("residual_join_u16", "dsic_residual_join_u16")
    total = 9 * RC * TILE * TILE // 8 * RN + 37
    _ab(c, "hi", lambda r: np.rint(_f(r, RN, RC, TILE, TILE, lo=-255.0, hi=255.0)))
    _ab(c, "blob", lambda r: r.integers(0, 256, total, dtype=np.uint8))
    c.inp("plane_off", np.array([5, 4000], dtype=np.int64), np.array([3001, 18], dtype=np.int64), bound=(0, total))
    c.inp("k", np.array([3, 7], dtype=np.int32), np.array([5, 0], dtype=np.int32), bound=(0, 10))
    c.out("q", F32, RN * RC * TILE * TILE)
    c.call = lambda L, p, s: L.dsic_residual_join_u16(p.hi, p.blob, total, p.plane_off, p.k, RN, RC, TILE, TILE, 40,
                                                      p.q, s)
    return c


# ---- overviews -------------------------------------------------------------------------------------------------
H2, W2 = (IH + 1) // 2, (IW + 1) // 2
HO, WO = 41, 67                                  # odd sides: the last row and column count twice
HO2, WO2 = 21, 34


def _validity(H, W):
    def make(r):
        v = (r.random((H, W)) < 0.7).astype(np.uint8) * r.integers(1, 256, (H, W), dtype=np.uint8)
        v[:6, :9] = 0
        return v
    return make


def _halve(kind, valid, C=3):
    export = "dsic_image_halve_" + ("valid_" if valid else "") + kind
    name = export[5:] + ("" if C == 3 else f"_c{C}")      # the kernels are instantiated per channel count

    def make(L):
        c = Case(name, export)
        fn = getattr(L, export)
        if kind == "f32":
            _ab(c, "src", lambda r: _f(r, C, HO, WO))
            c.out("dst", F32, C * HO2 * WO2)
            c.call = lambda L, p, s: fn(p.src, p.dst, C, HO, WO, s)
            return c
        dt = np.uint8 if kind == "u8" else np.uint16
        _ab(c, "src", lambda r: r.integers(0, 256 if kind == "u8" else 65536, (HO, WO, C), dtype=dt))
        c.out("dst", dt, C * HO2 * WO2)
        if valid:
            _ab(c, "sv", _validity(HO, WO))
            c.out("dv", U8, HO2 * WO2)
            c.call = lambda L, p, s: fn(p.src, p.sv, p.dst, p.dv, HO, WO, C, s)
        else:
            c.call = lambda L, p, s: fn(p.src, p.dst, HO, WO, C, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


for _k, _v in (("u8", False), ("f32", False), ("u16", False), ("u8", True), ("u16", True)):
    _halve(_k, _v)
for _c in (1, 2, 4):
    _halve("u8", False, _c)
    _halve("u16", False, _c)
    _halve("u8", True, _c)
    _halve("u16", True, _c)


# ---- nodata and validity masks ---------------------------------------------------------------------------------
NODATA = 7
PLANE_DW = TILE * TILE // 32


def _masked_img(C):
    def make(r):
        img = r.integers(0, 256, (IH, IW, C), dtype=np.uint8)
        hole = r.random((IH, IW)) < 0.2
        hole[:12, :40] = True
        img[hole] = NODATA
        return img
    return make


def _classify(name, valid, C=3):
    def make(L):
        c = Case(name, "dsic_valid_classify" if valid else "dsic_mask_classify_u8")
        c.out("counts", I32, N_TILES, zero=True)
        if valid:
            _ab(c, "v", _validity(IH, IW))
            c.call = lambda L, p, s: L.dsic_valid_classify(p.v, IH, IW, TILE, TILE, 0, N_TILES, p.counts, s)
        else:
            _ab(c, "img", _masked_img(C))
            c.call = lambda L, p, s: L.dsic_mask_classify_u8(p.img, IH, IW, C, TILE, TILE, NODATA, 0, N_TILES,
                                                             p.counts, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_classify("mask_classify_u8", False)
_classify("mask_classify_u8_c4", False, 4)
_classify("valid_classify", True)


def _delta(name, valid, C=3):
    def make(L):
        c = Case(name, "dsic_valid_delta_planes" if valid else "dsic_mask_delta_planes_u8")
        _ids(c, N_TILES)
        c.out("planes", U32, N_TILES * PLANE_DW)
        c.out("pop", I32, N_TILES, zero=True)
        if valid:
            _ab(c, "v", _validity(IH, IW))
            c.call = lambda L, p, s: L.dsic_valid_delta_planes(p.v, IH, IW, TILE, TILE, p.ids, N_TILES, p.planes,
                                                               p.pop, s)
        else:
            _ab(c, "img", _masked_img(C))
            c.call = lambda L, p, s: L.dsic_mask_delta_planes_u8(p.img, IH, IW, C, TILE, TILE, NODATA, p.ids, N_TILES,
                                                                 p.planes, p.pop, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_delta("mask_delta_planes_u8", False)
_delta("mask_delta_planes_u8_c4", False, 4)
_delta("valid_delta_planes", True)


def _planes_ab(n):
    """two sets of bit planes whose popcounts agree tile by tile (B holds A's words in another order): tile 0 sparse
    (its payload is a list of positions), tile 1 dense (the plane itself), the others in between"""
    r = _rng("planes", "A")
    A = np.zeros((n, PLANE_DW), dtype=np.uint32)
    for t in range(n):
        density = (0.01, 0.5, 0.03, 0.2, 0.0, 0.06)[t % 6]
        bits = r.random((PLANE_DW, 32)) < density
        A[t] = (bits * (1 << np.arange(32, dtype=np.uint64))).sum(1).astype(np.uint32)
    B = np.roll(A, 5, axis=1)
    pop = np.array([[bin(int(w)).count("1") for w in row] for row in A]).sum(1).astype(np.int32)
    return A, B, pop


@recipe
def mask_pack(L):
    c = Case("mask_pack", "dsic_mask_pack")
    n = 4
    A, B, pop = _planes_ab(n)
    c.inp("planes", A, B)
    c.same("pop", pop, bound=(0, TILE * TILE + 1))
    c.same("ids", np.array([0, 2, 3, 5], dtype=np.int32), bound=(0, N_TILES))
    c.work("ws", I64, n + 2)
    c.out("out", U8, n * (12 + TILE * TILE // 8))
    c.call = lambda L, p, s: L.dsic_mask_pack(p.planes, p.pop, p.ids, n, TILE, TILE, p.ws, p.out, s)

    def reach(L):
        assert 2 * pop[0] < TILE * TILE // 8 <= 2 * pop[1]          # both payload modes
    c.reach = reach
    return c


@recipe
def mask_unpack(L):
    c = Case("mask_unpack", "dsic_mask_unpack")
    nbytes, npos = TILE * TILE // 8, 20
    blobs = []
    for w in ("A", "B"):
        r = _rng("unpack", w)
        plane = r.integers(0, 256, nbytes, dtype=np.uint8)
        pos = np.sort(r.choice(TILE * TILE, npos, replace=False)).astype("<u2")
        blobs.append(np.concatenate([np.full(3, 0x99, np.uint8), plane, pos.view(np.uint8),
                                     np.full(17, 0x99, np.uint8)]))
    c.inp("blob", *blobs)
    total = blobs[0].size // 4 * 4
    c.same("desc", np.array([[0, 3, nbytes], [1, 3 + nbytes, 2 * npos]], dtype=np.int32), bound=(0, total))
    c.out("planes", U32, 2 * PLANE_DW)
    c.call = lambda L, p, s: L.dsic_mask_unpack(p.blob, total, p.desc, 2, TILE, TILE, p.planes, s)
    return c


def _apply(name, kind):
    def make(L):
        c = Case(name, "dsic_" + name)
        n = 4
        A, B, _ = _planes_ab(n)
        c.inp("planes", A, B)
        # (tile, plane or -1 for "all set"): any tile and plane number is legal, one outside writes nothing
        c.inp("desc", np.array([[0, 0], [1, 1], [2, -1], [4, 3]], dtype=np.int32),
              np.array([[0, 1], [1, 0], [3, -1], [5, 2]], dtype=np.int32), bound=(-1, N_TILES))
        wy, wx, wh, ww = WIN
        geo = (IH, IW, 3, TILE, TILE, wy, wx, wh, ww)
        fn = getattr(L, "dsic_" + name)
        if kind == "win":
            c.out("out", U8, wh * ww)
            c.call = lambda L, p, s: fn(p.planes, n, p.desc, 4, p.out, IH, IW, TILE, TILE, wy, wx, wh, ww, s)
        else:
            c.out("out", {"u8": U8, "u16": U16, "f32": F32}[kind], 3 * wh * ww)
            c.call = lambda L, p, s: fn(p.planes, n, p.desc, 4, NODATA, p.out, *geo, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


_apply("mask_apply_u8", "u8")
_apply("mask_apply_f32", "f32")
_apply("mask_apply_u16", "u16")
_apply("mask_window_u8", "win")


# ---- 16-bit scale ----------------------------------------------------------------------------------------------
def _band_range(name, valid, none=False, C=3):
    def make(L):
        c = Case(name, "dsic_band_range_valid_u16" if valid else "dsic_band_range_u16")
        H, W = 150, 200                          # more pixels than one workgroup takes: init, partial ranges, finish
        _ab(c, "img", lambda r: r.integers(300, 60000, (H, W, C)).astype(np.uint16))
        c.out("lohi", U32, 2 * C)
        if valid:
            if none:                             # set A has no valid pixel: only the finish launch makes its (0, 0)
                c.inp("v", np.zeros((H, W), dtype=np.uint8), _validity(H, W)(_rng(name, "B")))
            else:
                _ab(c, "v", _validity(H, W))
            c.call = lambda L, p, s: L.dsic_band_range_valid_u16(p.img, p.v, H, W, C, p.lohi, s)

            def restate(i):
                px = i["img"][i["v"] != 0]
                if not len(px):
                    return bytes(8 * C)
                return np.stack([px.min(0), px.max(0)], 1).astype(np.uint32).tobytes()
        else:
            c.call = lambda L, p, s: L.dsic_band_range_u16(p.img, H, W, C, p.lohi, s)

            def restate(i):
                px = i["img"].reshape(-1, C)
                return np.stack([px.min(0), px.max(0)], 1).astype(np.uint32).tobytes()
        c.restate = restate
        return c
    make.__name__ = name
    RECIPES.append(make)


_band_range("band_range_u16", False)
_band_range("band_range_valid_u16", True)
_band_range("band_range_valid_u16_none", True, none=True)
for _c in (1, 2, 4):                             # one launch statement per channel count
    _band_range(f"band_range_u16_c{_c}", False, C=_c)
    _band_range(f"band_range_valid_u16_c{_c}", True, C=_c)


# ---- resampled, rendered and warped reads ----------------------------------------------------------------------
REGION = (3, 5, 30, 60)                          # y0, x0, h, w of the 40 x 70 source at shift 0
OH, OW = 11, 23


def _view_src(c, kind, C, valid):
    if kind == "f32":
        _ab(c, "src", lambda r: _f(r, C, IH, IW))
    else:
        _ab(c, "src", _img(np.uint8 if kind == "u8" else np.uint16, C))
    if valid:
        _ab(c, "sv", _validity(IH, IW))


def _resample(kind, valid):
    name = "window_resample_" + ("valid_" if valid else "") + kind

    def make(L):
        c = Case(name, "dsic_" + name)
        C = 3
        _view_src(c, kind, C, valid)
        c.out("dst", {"u8": U8, "u16": U16, "f32": F32}[kind], C * OH * OW)
        fn = getattr(L, "dsic_" + name)
        geo = (IH, IW, 0, 0, C, 0, *REGION)
        if valid:
            c.out("dv", U8, OH * OW)
            c.call = lambda L, p, s: fn(p.src, p.sv, *geo, p.dst, p.dv, OH, OW, 0, 9, s)
        elif kind == "f32":
            c.call = lambda L, p, s: fn(p.src, *geo, p.dst, OH, OW, 0, 0.0, 0, s)
        else:
            c.call = lambda L, p, s: fn(p.src, *geo, p.dst, OH, OW, 0, -1, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


for _k, _v in (("u8", False), ("u16", False), ("f32", False), ("u8", True), ("u16", True)):
    _resample(_k, _v)


def _display(c, kind):
    c.hostarr("bands", ctypes.c_int, [2, 0, 1])
    top = 255 if kind == "u8" else 65535
    c.hostarr("lohi8", ctypes.c_uint32, [10, top - 20, 0, top, 30, top // 2])


def _render(kind, valid=True):
    export = "dsic_window_render_" + kind
    name = export[5:] + ("" if valid else "_all_valid")   # with and without a validity window: two launch statements

    def make(L):
        c = Case(name, export)
        _view_src(c, kind, 3, valid)
        _display(c, kind)
        c.out("dst", U8, OH * OW * 4)
        fn = getattr(L, export)
        c.call = lambda L, p, s: fn(p.src, p.sv if valid else None, IH, IW, 0, 0, 3, 0, *REGION, p.bands, 3, p.lohi8, p.dst, OH, OW, 0,
                                    -1, 1, 17, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


for _k in ("u8", "u16"):
    _render(_k)
    _render(_k, False)


def _histogram(kind):
    name = "band_histogram_" + kind

    def make(L):
        c = Case(name, "dsic_" + name)
        C = 3 if kind == "u8" else 1
        _ab(c, "img", _img(np.uint8 if kind == "u8" else np.uint16, C))
        _ab(c, "v", _validity(IH, IW))
        c.out("hist", U32, C * (256 if kind == "u8" else 65536), zero=True)
        fn = getattr(L, "dsic_" + name)
        c.call = lambda L, p, s: fn(p.img, p.v, IH, IW, C, -1, p.hist, s)

        def restate(i):
            px = i["img"][i["v"] != 0]
            return np.stack([np.bincount(px[:, ch], minlength=256 if kind == "u8" else 65536)
                             for ch in range(C)]).astype(np.uint32).tobytes()
        c.restate = restate
        return c
    make.__name__ = name
    RECIPES.append(make)


_histogram("u8")
_histogram("u16")

WARP_M = [2 << 16, 3 << 12, 1 << 16, -(3 << 12), 2 << 16, 4 << 16]     # two level-0 pixels per output pixel, a slight turn
WOH, WOW = 18, 30


def _warp(kind, render, valid=True):
    export = "dsic_window_warp_" + ("render_" if render else "") + kind
    name = export[5:] + ("" if valid else "_all_valid")

    def make(L):
        c = Case(name, export)
        _view_src(c, kind, 3, valid)
        c.hostarr("m", ctypes.c_int64, WARP_M)
        fn = getattr(L, export)
        sv = (lambda p: p.sv) if valid else (lambda p: None)
        geo = (IH, IW, 0, 0, 3, 0, IH, IW, IH, IW)
        if render:
            _display(c, kind)
            c.out("dst", U8, WOH * WOW * 4)
            c.call = lambda L, p, s: fn(p.src, sv(p), *geo, p.m, p.bands, 3, p.lohi8, p.dst, WOH, WOW, 2, -1, 1, 17, s)
        else:
            c.out("dst", U8 if kind == "u8" else U16, WOH * WOW * 3)
            c.out("dv", U8, WOH * WOW)
            c.call = lambda L, p, s: fn(p.src, sv(p), *geo, p.m, p.dst, p.dv, WOH, WOW, 2, -1, 9, s)
        return c
    make.__name__ = name
    RECIPES.append(make)


for _k in ("u8", "u16"):
    for _v in (True, False):
        _warp(_k, False, _v)
        _warp(_k, True, _v)


# ---- the table --------------------------------------------------------------------------------------------------
_BUILT = {}


def names():
    return [fn.__name__ for fn in RECIPES]


def build(name, L):
    """the Case of one recipe (built once; its arrays are read-only)"""
    if name not in _BUILT:
        fn = next(f for f in RECIPES if f.__name__ == name)
        c = fn(L)
        assert c.name == name and c.call is not None, name
        for b in c.bufs.values():
            if b["kind"] == "in":
                b["A"].setflags(write=False)
                b["B"].setflags(write=False)
        _BUILT[name] = c
    return _BUILT[name]


FAMILIES = {"weights": ("pack_", "split_wino"), "layout": ("image_to_", "nhwc_", "nchw_", "reflect", "normalize",
                                                           "image_u8hwc"),
            "conv": ("conv",), "rate": ("hyper", "rate", "sigma_nu", "student", "gaussian", "round", "gdn"),
            "metrics": ("ssim", "avgpool", "msssim", "sqerr"),
            "coder": ("latent", "cdf_", "range_"), "container": ("container", "strings_"),
            "tiles": ("tile_",), "residual": ("residual",), "overviews": ("image_halve",),
            "masks": ("mask_", "valid_"), "scale": ("band_range",),
            "views": ("window_", "band_histogram")}


def family(name):
    for fam, heads in FAMILIES.items():
        if name.startswith(heads):
            return fam
    raise KeyError(name)
