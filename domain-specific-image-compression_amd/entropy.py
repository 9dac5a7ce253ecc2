"""Mirror of code/modelv2/eval_selfcontained_entropy.py: custom_compress /
custom_decompress / evaluate-style helpers, running on the GPU.

The reference script is a sketch that cannot execute (StudentT.cdf is not
implemented in torch; torchac is called with arguments it does not accept —
SURVEY.md §8c).  This module keeps its interface — the returned dict of :68-74,
`tail=10`, z string then y string per image, decode order of :76-123 — and the
interpretation frozen in DESIGN.md "Entropy path".
"""
from __future__ import annotations

import ctypes
import os
import struct

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .ops import _f32c, _p, _stream

DEFAULT_LMAX = 256
# The range encoder runs as pack -> chain -> place (dsic_range_encode_ws: the serial chain is a wave of 8 VGPRs that
# shares its CU with a persistent conv workgroup); DSIC_SPLIT_CODER=0 keeps the single kernel (A/B runs).
SPLIT_CODER = os.environ.get("DSIC_SPLIT_CODER", "1") != "0"


class EntropyError(RuntimeError):
    pass


def _check_err(err, what):
    _raise_err(int(err.item()), what)


def _raise_err(code, what):
    if code:
        reasons = [m for bit, m in ((1, "support wider than Lmax"), (2, "symbol outside its support"),
                                    (4, "output capacity exceeded")) if code & bit]
        raise EntropyError(f"{what}: " + ", ".join(reasons))


def gaussian_cdf(x):
    """:14-15 in float32, like the reference's CPU torch evaluation (host, through the
    library's own table math: x / float(sqrt 2), erf, 1 + ., 0.5 * .)."""
    L = _lib.load()
    a = np.asarray(x, dtype=np.float32)
    return np.array([L.dsic_host_gaussian_cdf_f32(float(v)) for v in a.ravel()], dtype=np.float32).reshape(a.shape)


def pmf_to_uint16_cdf(pmf):
    """:17-23 on the host: pmf [L, C, ...] float32 (support axis first) -> uint16 [L+1, C, ...]."""
    L = _lib.load()
    p = np.ascontiguousarray(np.asarray(pmf, dtype=np.float32))
    Ls = p.shape[0]
    C = int(np.prod(p.shape[1:], dtype=np.int64)) if p.ndim > 1 else 1
    out = np.empty((Ls + 1, C), dtype=np.uint16)
    _lib.check(L.dsic_host_pmf_to_uint16_cdf(p.ctypes.data_as(ctypes.c_void_p), Ls, C,
                                             out.ctypes.data_as(ctypes.c_void_p)), "pmf_to_uint16_cdf")
    return out.reshape((Ls + 1,) + p.shape[1:])


def sigma_z_of(model):
    """:32 `torch.exp(model.z_prior.log_sigma)` (no clamp), evaluated on the host by the
    library's deterministic exp (float32 of the float64 value) so that an encoder and a decoder
    on different machines build the same z tables; returned on the model's device."""
    L = _lib.load()
    ls = model.z_prior.log_sigma.detach()
    vals = np.array([L.dsic_host_exp_f32(float(v)) for v in ls.cpu().numpy().astype(np.float32).ravel()],
                    dtype=np.float32)
    return torch.from_numpy(vals).to(ls.device)


def latent_support(y_tilde, z_tilde, tail=10):
    """-> meta int32 [B,4] = (ymin-tail, Ly, zmin-tail, Lz) on the device (:39-41, :52-54)."""
    y = _f32c(y_tilde, "latent_support")
    z = _f32c(z_tilde, "latent_support")
    B = y.shape[0]
    meta = torch.empty((B, 4), dtype=torch.int32, device=y.device)
    _lib.check(_lib.load().dsic_latent_support(_p(y), _p(z), _p(meta), B, y[0].numel(), z[0].numel(), int(tail),
                                               _stream()), "latent_support")
    return meta


def cdf_tables(sigma_y, nu_y, sigma_z, meta, Lmax=DEFAULT_LMAX, err=None):
    """-> (tab_y [B,rows,Lmax], tab_z [B,N,Lmax]) uint16 coder tables (:43-47, :55-61, :17-23).

    sigma_y/nu_y: [B,M] (one row per channel) or [B,M,Hy,Wy] (spatial_params: one row per latent
    element, NCHW order = symbol order)."""
    sy = _f32c(sigma_y, "cdf_tables").reshape(sigma_y.shape[0], -1)
    ny = _f32c(nu_y, "cdf_tables").reshape(nu_y.shape[0], -1)
    sz = _f32c(sigma_z, "cdf_tables")
    B, M = sy.shape
    N = sz.numel()
    dev = sy.device
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    # entries k >= L_b of a row are never read (every reader stops at the support width in `meta`)
    tab_y = torch.empty((B, M, Lmax), dtype=torch.uint16, device=dev)
    tab_z = torch.empty((B, N, Lmax), dtype=torch.uint16, device=dev)
    L = _lib.load()
    _lib.check(L.dsic_cdf_tables_gauss(_p(sz), _p(meta), _p(tab_z), B, N, Lmax, _p(err), _stream()),
               "cdf_tables_gauss")
    _lib.check(L.dsic_cdf_tables_student(_p(sy), _p(ny), _p(meta), _p(tab_y), B, M, Lmax, _p(err), _stream()),
               "cdf_tables_student")
    return tab_y, tab_z, err


def _cap(n):
    return (2 * n + 16 + 3) // 4 * 4   # <= 16 bits per symbol + flush, multiple of 4


SEGMENTS = (1, 2, 4, 8, 16)


def check_segments(segments, M, what):
    """segments as an int: one of SEGMENTS that divides the M channels of y, else ValueError."""
    try:
        K = int(segments)
    except (TypeError, ValueError):
        K = -1
    if K != segments or K not in SEGMENTS or int(M) % K:
        raise ValueError(f"{what}: segments={segments!r} must be one of {SEGMENTS} and divide M={M}")
    return K


@torch.no_grad()
def compress_latents(y_tilde, z_tilde, sigma_y, nu_y, sigma_z, tail=10, Lmax=DEFAULT_LMAX, streams_per_wg=1,
                     split=None, segments=1):
    """Device-resident compress of already computed latents.

    y_tilde [B,M,Hy,Wy], z_tilde [B,N,Hz,Wz] integer-valued (quant_mode="round");
    sigma_y/nu_y [B,M]; sigma_z [N].  Returns dict with device tensors:
    bytes uint8 [B, cap_z+cap_y], lengths int32 [B,2] (z,y), meta int32 [B,4],
    cap_z, cap_y, tab_y, tab_z, err.  Nothing synchronises with the host.
    split: the split encoder (default SPLIT_CODER; streams_per_wg > 1 always uses the single kernel).
    segments = K > 1 (one of SEGMENTS, dividing M; the split encoder only): the y string of an image is coded as K
    independent strings, one per group of M / K channels, with the same support and tables.  Then bytes is
    [B, cap_z + K * cap_y] with segment k at cap_z + k * cap_y (cap_y the capacity of one segment) and lengths is
    [B, 1 + K] (z, y segment 0 .. K - 1); the dict carries "segments" either way.
    """
    y = _f32c(y_tilde, "compress")
    z = _f32c(z_tilde, "compress")
    B, M, Hy, Wy = y.shape
    _, N, Hz, Wz = z.shape
    dev = y.device
    K = check_segments(segments, M, "compress_latents")
    use_split = bool(SPLIT_CODER if split is None else split) and int(streams_per_wg) == 1
    if K > 1 and not use_split:
        raise ValueError("compress_latents: segments > 1 needs the split encoder (split=False, DSIC_SPLIT_CODER=0 or "
                         "streams_per_wg > 1 select the single kernel, which codes whole strings)")
    per_element = sigma_y.dim() == 4        # spatial_params: a table row per latent element
    meta = latent_support(y, z, tail)
    tab_y, tab_z, err = cdf_tables(sigma_y, nu_y, sigma_z, meta, Lmax)
    cap_y, cap_z = _cap(M * Hy * Wy // K), _cap(N * Hz * Wz)
    # the coder ORs its bits in: zero-filled, as 32-bit words (a byte fill kernel takes 4x the elements)
    out = torch.zeros((B, (cap_z + K * cap_y) // 4), dtype=torch.int32, device=dev).view(torch.uint8)
    lengths = torch.zeros((B, 1 + K), dtype=torch.int32, device=dev)
    L = _lib.load()
    if use_split:
        # K = 1 is dsic_range_encode_ws's launches.  The caching allocator on the coder's stream: every call in
        # flight has its own workspace
        nbytes = L.dsic_range_encode_seg_workspace_size(B, M, Hy * Wy, N, Hz * Wz, K)
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=dev)
        _lib.check(L.dsic_range_encode_seg_ws(_p(y), _p(z), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, M, Hy * Wy,
                                              N, Hz * Wz, _p(out), cap_y, cap_z, _p(lengths), _p(err),
                                              int(per_element), K, _p(ws), ws.numel() * 4, _stream()),
                   "range_encode_seg_ws")
    else:
        _lib.check(L.dsic_range_encode(_p(y), _p(z), _p(meta), _p(tab_y), _p(tab_z), Lmax, B, M, Hy * Wy,
                                       N, Hz * Wz, _p(out), cap_y, cap_z, _p(lengths), _p(err),
                                       int(streams_per_wg), int(per_element), _stream()), "range_encode")
    return {"bytes": out, "lengths": lengths, "meta": meta, "cap_z": cap_z, "cap_y": cap_y, "segments": K,
            "tab_y": tab_y, "tab_z": tab_z, "err": err, "shape_y": list(y.shape), "shape_z": list(z.shape)}


def masked_streams(coder_cus=16, total_cus=256, xcds=8):
    """(main, coder) torch ExternalStreams on disjoint CU sets.

    The coder gets coder_cus/xcds CUs of EVERY XCD (workgroups are dealt round-robin over the
    XCDs, so removing CUs from one XCD only would make it the straggler of every conv launch).
    The pattern k*32+j with j = k, k+8, ... selects the same number of CUs per XCD whether mask
    bits enumerate CUs XCD-major or XCD-interleaved."""
    L = _lib.load()
    words = (total_cus + 31) // 32
    per_xcd = max(1, coder_cus // xcds)
    bits = np.zeros(total_cus, dtype=bool)
    for k in range(xcds):
        for t in range(per_xcd):
            bits[k * (total_cus // xcds) + (k + 8 * t) % (total_cus // xcds)] = True

    def make(sel):
        m = np.zeros(words, dtype=np.uint32)
        for i in np.nonzero(sel)[0]:
            m[i // 32] |= np.uint32(1 << (i % 32))
        h = ctypes.c_void_p()
        _lib.check(L.dsic_stream_create_masked(m.ctypes.data_as(ctypes.c_void_p), words, ctypes.byref(h)),
                   "stream_create_masked")
        return torch.cuda.ExternalStream(h.value)

    return make(~bits), make(bits)


class AsyncCompressor:
    """Runs compress_latents on side HIP streams so that the serial range coder overlaps
    synthesis (and the following batches' analysis).  Use as the `after_rate` hook of
    CompressionModel.forward; call .wait() before reading `.last`.

    `depth` side streams are used round-robin: the coder of batch i+1 does not queue behind the
    coder of batch i, so a coder that takes longer than one step (512x512 patches: 196 608 y symbols
    per string, a serial chain) still keeps up - its latency is hidden, its throughput doubles."""

    def __init__(self, model, tail=10, Lmax=DEFAULT_LMAX, stream=None, streams_per_wg=1, depth=1, segments=1):
        self.model, self.tail, self.Lmax = model, tail, Lmax
        self.streams_per_wg = streams_per_wg
        self.segments = check_segments(segments, model.M, "AsyncCompressor")   # y segments (compress_latents)
        self.streams = [stream if stream is not None else torch.cuda.Stream()]
        self.streams += [torch.cuda.Stream() for _ in range(max(1, int(depth)) - 1)]
        self.stream = self.streams[0]
        self.calls = 0
        self.last = None
        self._sigma_z = None
        self.timing = False          # bench.py: keep a HIP-event pair per call on the coder's stream
        self.times = []
        self._events = []            # pre-created timing events (see reserve_events)
        self._ready = None

    def reserve_events(self, n):
        """create n (start, done) timing-event pairs now, so that none is created while timing"""
        with torch.cuda.stream(self.stream):
            while len(self._events) < n:
                pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                pair[0].record(self.stream)
                pair[1].record(self.stream)
                self._events.append(pair)

    def _pair(self):
        if self._events:
            return self._events.pop()
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __call__(self, partial):
        main = torch.cuda.current_stream()
        side = self.streams[self.calls % len(self.streams)]
        self.calls += 1
        if self._sigma_z is None:
            self._sigma_z = sigma_z_of(self.model)
            for st in self.streams:
                self._sigma_z.record_stream(st)
        if self._ready is None:
            self._ready = torch.cuda.Event()
        ready = self._ready              # re-recorded per call; wait_event captures this record
        ready.record(main)
        tensors = [partial["y_tilde"], partial["z_tilde"], partial["sigma"], partial["nu"]]
        with torch.cuda.stream(side):
            side.wait_event(ready)
            for t in tensors:
                t.record_stream(side)             # allocator must not recycle them under the coder
            if self.timing:
                e0, done = self._pair()
                e0.record(side)
            else:
                done = torch.cuda.Event()
            self.last = compress_latents(tensors[0], tensors[1], tensors[2], tensors[3], self._sigma_z,
                                         self.tail, self.Lmax, self.streams_per_wg, segments=self.segments)
            done.record(side)
            if self.timing:
                self.times.append((e0, done))
            self.last["done"] = done

    def wait(self):
        for st in self.streams:
            torch.cuda.current_stream().wait_stream(st)
        return self.last


def _per_channel(t):
    """[B,M,H,W] spatially constant (expanded) -> contiguous [B,M]; per-element tensors
    (spatial_params) and [B,M] pass through."""
    if t.dim() == 4 and t.stride(2) == 0 and t.stride(3) == 0:
        return t[:, :, 0, 0].contiguous()
    return t.contiguous()


def _tight_lmax(meta, minimum=32):
    """Support width of this batch (host sync): keeps per-element tables small."""
    L = int(meta[:, [1, 3]].max().item())
    return max(minimum, (L + 7) // 8 * 8)


TABLE_FLOW_VERSION = 2     # 1: float64 tables (round 1); 2: float32 CPU-torch operation order


def numerics_tag() -> int:
    """What a decoder must share with the encoder to rebuild the same coder tables: the table flow, and the
    arithmetic of the kernels that recompute sigma / nu from the decoded z (h_s: code/modelv2/
    eval_selfcontained_entropy.py:100-106).  bits 0-7 table flow version, bit 8 split-bf16 Winograd kernels
    (DSIC_WINO_BF16), bit 9 Winograd at all (DSIC_WINOGRAD), bits 16-31 the library's ABI version.  A stream carries
    the tag of its encoder; custom_decompress refuses a stream whose tag is not its own."""
    from . import layers as _layers
    return (TABLE_FLOW_VERSION | (int(bool(_layers.WINO_BF16)) << 8) | (int(bool(_layers.USE_WINOGRAD)) << 9)
            | ((int(_lib.load().dsic_abi_version()) & 0xFFFF) << 16))


def _coded_batch(model, x, tail, Lmax, what, pack=False, segments=1):
    """forward(round) and the range coder of custom_compress, with its Lmax retry.  pack=True also writes the DSIC2
    container on the device (_pack_on_device) and learns the error word with the container's size, one copy."""
    segments = check_segments(segments, model.M, what)
    out = model(x, quant_mode="round")
    sigma_z = sigma_z_of(model)                                        # :32 (no clamp)
    if getattr(model, "spatial_params", False):
        # one table row per latent element: size the rows to the actual support (the reference
        # reads min/max on the host here too, :39-40,52-53)
        Lmax = min(1000, _tight_lmax(latent_support(out["y_tilde"], out["z_tilde"], tail)))
    while True:
        c = compress_latents(out["y_tilde"], out["z_tilde"], _per_channel(out["sigma"]),
                             _per_channel(out["nu"]), sigma_z, tail, Lmax, segments=segments)
        c["x_hat"] = out["x_hat"]                                      # the forward reconstruction (codec's residual layer)
        if pack:
            c["container"], c["container_bytes"], code = _pack_on_device(c, numerics_tag())
        else:
            code = int(c["err"].item())
        try:
            _raise_err(code, what)
            return c
        except EntropyError:
            if Lmax >= 1000 or not (code & 1):
                raise
            Lmax = min(1000, Lmax * 2)                                 # wider support than expected


@torch.no_grad()
def custom_compress(model, x, tail=10, Lmax=DEFAULT_LMAX, segments=1):
    """eval_selfcontained_entropy.py:26-74.  Returns the reference's dict:
    strings [[z_bytes, y_bytes], ...], shape_y, shape_z, min_y, max_y, min_z, max_z.
    segments = K > 1: y_bytes is the K segment strings of compress_latents joined, and the dict gains "segments" and
    "seg_lengths_y" (per image the K lengths)."""
    c = _coded_batch(model, x, tail, Lmax, "custom_compress", segments=segments)
    K = c["segments"]
    lengths = c["lengths"].cpu().numpy()
    meta = c["meta"].cpu().numpy()
    raw = c["bytes"].cpu().numpy()
    strings = []
    for b in range(raw.shape[0]):
        zs = raw[b, :lengths[b, 0]].tobytes()
        ys = b"".join(raw[b, c["cap_z"] + k * c["cap_y"]:c["cap_z"] + k * c["cap_y"] + lengths[b, 1 + k]].tobytes()
                      for k in range(K))
        strings.append([zs, ys])
    seg = {"segments": K, "seg_lengths_y": [[int(v) for v in lengths[b, 1:]] for b in range(raw.shape[0])]}
    return {
        **(seg if K > 1 else {}),
        "strings": strings,
        "shape_y": c["shape_y"], "shape_z": c["shape_z"],
        "min_y": [int(m[0]) for m in meta], "max_y": [int(m[0] + m[1] - 1) for m in meta],
        "min_z": [int(m[2]) for m in meta], "max_z": [int(m[2] + m[3] - 1) for m in meta],
        "numerics": numerics_tag(),        # beyond the reference's keys (:68-74): see numerics_tag()
    }


def _upload_strings(strings, which, dev):
    lens = [len(s[which]) for s in strings]
    stride = max(4, (max(lens) + 3) // 4 * 4)
    buf = np.zeros((len(strings), stride), dtype=np.uint8)
    for b, s in enumerate(strings):
        buf[b, :lens[b]] = np.frombuffer(s[which], dtype=np.uint8)
    return (torch.from_numpy(buf).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), stride)


def _refuse_tag(tag, what):
    if tag is not None and int(tag) != numerics_tag():
        raise EntropyError(f"{what}: the stream was written with numerics tag {int(tag):#x}, this decoder "
                           f"is {numerics_tag():#x} (table flow / kernel arithmetic differ: the coder tables would "
                           "not match and the latents would decode to garbage)")


def _dict_segments(compressed, what):
    """(K, per image the K segment lengths) of a custom_compress dict; ValueError where they contradict its strings."""
    K = check_segments(compressed.get("segments", 1), compressed["shape_y"][1], what)
    if K == 1:
        return 1, [[len(s[1])] for s in compressed["strings"]]
    seg = [[int(v) for v in row] for row in compressed["seg_lengths_y"]]
    if len(seg) != len(compressed["strings"]) or any(
            len(row) != K or min(row) < 0 or sum(row) != len(s[1]) for row, s in zip(seg, compressed["strings"])):
        raise ValueError(f"{what}: seg_lengths_y must hold {K} lengths per image that add up to its y string")
    return K, seg


def _default_lmax(model, meta_np):
    Lmax = int(meta_np[:, [1, 3]].max())
    return (Lmax + 7) // 8 * 8 if getattr(model, "spatial_params", False) else max(DEFAULT_LMAX, Lmax)


def _decode_batch(model, shape_y, shape_z, meta, Lmax, z, y, what, segments=1, seg_lengths=None):
    """:76-120 from strings already on the device: z / y = (buffer, stride, lengths, lstride, loff) as
    dsic_range_decode takes them; segments = K > 1: every y string is K segments back to back, seg_lengths the device
    int32 [B, K] of their lengths (dsic_range_decode_seg).  Returns g_s's output, not yet clamped."""
    dev = meta.device
    B, M, Hy, Wy = shape_y
    _, N, Hz, Wz = shape_z
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _lib.load()
    sigma_z = sigma_z_of(model)
    tab_z = torch.zeros((B, N, Lmax), dtype=torch.uint16, device=dev)
    _lib.check(L.dsic_cdf_tables_gauss(_p(sigma_z), _p(meta), _p(tab_z), B, N, Lmax, _p(err), _stream()),
               "cdf_tables_gauss")
    zbuf, zstride, zlen, zls, zlo = z
    z_hat = torch.empty((B, N, Hz, Wz), dtype=torch.float32, device=dev)
    _lib.check(L.dsic_range_decode(_p(zbuf), zstride, _p(zlen), zls, zlo, _p(meta), 2, _p(tab_z), Lmax, B, N,
                                   Hz * Wz, 0, _p(z_hat), _p(err), _stream()), "range_decode(z)")
    # :100-106: hyper-synthesis on the decoded z
    (_, _, sigma_y, nu_y), _ = model.h_s.params_nhwc(ops.nchw_to_nhwc(z_hat), model.min_nu, model.max_nu)
    per_element = int(getattr(model, "spatial_params", False))
    rows = M * Hy * Wy if per_element else M
    tab_y = torch.zeros((B, rows, Lmax), dtype=torch.uint16, device=dev)
    _lib.check(L.dsic_cdf_tables_student(_p(sigma_y.contiguous()), _p(nu_y.contiguous()), _p(meta), _p(tab_y), B,
                                         rows, Lmax, _p(err), _stream()), "cdf_tables_student")
    ybuf, ystride, ylen, yls, ylo = y
    y_hat = torch.empty((B, M, Hy, Wy), dtype=torch.float32, device=dev)
    if segments > 1:
        _lib.check(L.dsic_range_decode_seg(_p(ybuf), ystride, _p(ylen), yls, ylo, _p(seg_lengths), segments, _p(meta),
                                           0, _p(tab_y), Lmax, B, M, Hy * Wy, per_element, _p(y_hat), _p(err),
                                           _stream()), "range_decode_seg(y)")
    else:
        _lib.check(L.dsic_range_decode(_p(ybuf), ystride, _p(ylen), yls, ylo, _p(meta), 0, _p(tab_y), Lmax, B, M,
                                       Hy * Wy, per_element, _p(y_hat), _p(err), _stream()), "range_decode(y)")
    _check_err(err, what)
    return model.g_s.forward_nhwc(ops.nchw_to_nhwc(y_hat))            # :120


@torch.no_grad()
def custom_decompress(model, compressed, Lmax=None):
    """eval_selfcontained_entropy.py:76-123: decode z, re-run h_s, decode y, run g_s, clamp."""
    dev = next(model.parameters()).device
    _refuse_tag(compressed.get("numerics"), "custom_decompress")
    strings = compressed["strings"]
    B = len(strings)
    meta_np = np.array([[compressed["min_y"][b], compressed["max_y"][b] - compressed["min_y"][b] + 1,
                         compressed["min_z"][b], compressed["max_z"][b] - compressed["min_z"][b] + 1]
                        for b in range(B)], dtype=np.int32)
    if Lmax is None:
        Lmax = _default_lmax(model, meta_np)
    meta = torch.from_numpy(meta_np).to(dev)
    K, seg = _dict_segments(compressed, "custom_decompress")
    zbuf, zlen, zstride = _upload_strings(strings, 0, dev)
    ybuf, ylen, ystride = _upload_strings(strings, 1, dev)
    seg_lengths = torch.tensor(seg, dtype=torch.int32, device=dev) if K > 1 else None
    x_hat = _decode_batch(model, compressed["shape_y"], compressed["shape_z"], meta, Lmax,
                          (zbuf, zstride, zlen, 1, 0), (ybuf, ystride, ylen, 1, 0), "custom_decompress", K,
                          seg_lengths)
    return x_hat.clamp(0, 1)                                           # :123


def real_bpp(compressed, H, W):
    """:148-149 — 8 * total bytes / (H*W), per batch."""
    total_bits = sum(len(s) * 8 for entry in compressed["strings"] for s in entry)
    return total_bits / float(H * W)


# ---- container: the reference keeps the compressed patch batch as an in-memory dict (:68-74);
# this is that dict as one byte string, so the strings can leave the process ------------------
_MAGIC = b"DSIC2\x00"      # DSIC1: rounds 1-2, no numerics tag (float64 / float32 tables both wrote it: not decodable
_MAGIC_V1 = b"DSIC1\x00"   # safely any more, refused)
_MAGIC_SEG = b"DSIC3\x00"  # DSIC3: segmented y strings (written only for segments > 1)
_HEAD = struct.Struct("<6sI7I")      # magic, numerics tag, B, My, Hy, Wy, Nz, Hz, Wz
_SEGS = struct.Struct("<I")          # DSIC3: segments per y string, behind the head
_REC = struct.Struct("<4i2I")        # per image: min_y, max_y, min_z, max_z, len_z, len_y


def pack_container(compressed) -> bytes:
    """dict of custom_compress -> bytes.  Layout (little endian):
    magic(6) | numerics tag (uint32, numerics_tag()) | B,My,Hy,Wy,Nz,Hz,Wz (7 x uint32) | per image:
    min_y,max_y,min_z,max_z (4 x int32), len_z,len_y (2 x uint32) | per image: z bytes, y bytes.
    A dict with "segments" = K > 1 becomes a DSIC3 container: magic "DSIC3\\0", segs (uint32) behind the head's
    fields, the same records (len_y = the sum of the image's segments), then B x K uint32 segment lengths in front of
    the strings (the y bytes are the segments back to back)."""
    B, My, Hy, Wy = compressed["shape_y"]
    _, Nz, Hz, Wz = compressed["shape_z"]
    tag = int(compressed.get("numerics", numerics_tag()))
    K, seg = _dict_segments(compressed, "pack_container")
    head = [_HEAD.pack(_MAGIC_SEG if K > 1 else _MAGIC, tag, B, My, Hy, Wy, Nz, Hz, Wz)]
    if K > 1:
        head.append(_SEGS.pack(K))
    body = []
    for b in range(B):
        zs, ys = compressed["strings"][b]
        head.append(_REC.pack(compressed["min_y"][b], compressed["max_y"][b], compressed["min_z"][b],
                              compressed["max_z"][b], len(zs), len(ys)))
        body += [zs, ys]
    if K > 1:
        head.append(struct.pack(f"<{B * K}I", *[v for row in seg for v in row]))
    return b"".join(head + body)


def read_container_segments(read_at, off, size):
    """The head, the records and (DSIC3) the segment lengths of the container that fills bytes [off, off + size) behind
    read_at(offset, n) (n bytes at an offset: a slice of a blob, or codec._Source.read_at); the strings are not read.
    Returns (tag, shape_y, shape_z, per image (min_y, max_y, min_z, max_z, z_off, z_len, y_off, y_len), segs, per
    image the segs lengths of its y segments), offsets as read_at counts them; a DSIC2 container has segs = 1 and
    [y_len] per image.  ValueError for a DSIC1 container, another magic, records that do not add up to size, a segs
    that is not allowed for My, and segment lengths that do not add up to their record's len_y."""
    head = read_at(off, min(size, _HEAD.size))
    if head[:6] == _MAGIC_V1:
        raise ValueError("DSIC1 container: written before the numerics tag existed (its coder tables may be the float64 "
                         "ones of round 1); re-encode")
    if len(head) < _HEAD.size or bytes(head[:6]) not in (_MAGIC, _MAGIC_SEG):
        raise ValueError("not a DSIC container")
    _, tag, B, My, Hy, Wy, Nz, Hz, Wz = _HEAD.unpack(head)
    K, recs = 1, off + _HEAD.size
    if bytes(head[:6]) == _MAGIC_SEG:
        word = read_at(recs, min(max(size - _HEAD.size, 0), _SEGS.size))
        if len(word) < _SEGS.size:
            raise ValueError("truncated or oversized DSIC container")
        (K,) = _SEGS.unpack(word)
        recs += _SEGS.size
        if K not in SEGMENTS[1:] or My % K:
            raise ValueError(f"DSIC3 container: segs={K} is not one of {SEGMENTS[1:]} dividing My={My}")
    table = 4 * B * K if K > 1 else 0
    if B < 1 or off + size < recs + _REC.size * B + table:
        raise ValueError("truncated or oversized DSIC container")
    pos, images = recs + _REC.size * B + table, []
    for min_y, max_y, min_z, max_z, len_z, len_y in _REC.iter_unpack(read_at(recs, _REC.size * B)):
        images.append((min_y, max_y, min_z, max_z, pos, len_z, pos + len_z, len_y))
        pos += len_z + len_y
    if pos != off + size:
        raise ValueError("truncated or oversized DSIC container")
    if K > 1:
        flat = struct.unpack(f"<{B * K}I", read_at(recs + _REC.size * B, table))
        seg = [list(flat[b * K:(b + 1) * K]) for b in range(B)]
        if any(sum(row) != r[7] for row, r in zip(seg, images)):
            raise ValueError("DSIC3 container: segment lengths do not add up to their record's len_y")
    else:
        seg = [[r[7]] for r in images]
    return tag, [B, My, Hy, Wy], [B, Nz, Hz, Wz], images, K, seg


def read_container_head(read_at, off, size):
    """read_container_segments without the segments: (tag, shape_y, shape_z, images) of a DSIC2 or DSIC3 container."""
    return read_container_segments(read_at, off, size)[:4]


def _blob_head(blob):
    return read_container_segments(lambda off, n: blob[off:off + n], 0, len(blob))


def unpack_container(blob: bytes):
    """Inverse of pack_container (DSIC2 and DSIC3)."""
    tag, shape_y, shape_z, images, K, seg = _blob_head(blob)
    return {**({"segments": K, "seg_lengths_y": seg} if K > 1 else {}),
            "strings": [[blob[r[4]:r[4] + r[5]], blob[r[6]:r[6] + r[7]]] for r in images],
            "shape_y": shape_y, "shape_z": shape_z,
            "min_y": [r[0] for r in images], "max_y": [r[1] for r in images],
            "min_z": [r[2] for r in images], "max_z": [r[3] for r in images], "numerics": tag}


# ---- the same container, written and read on the device (codec.py's batches) ----------------------------------
def _pack_on_device(c, tag):
    """compress_latents' outputs -> (DSIC2 container in a device buffer, its size, the coder's error word).  The size and
    the error word come back in one 16-byte copy; nothing is sliced per image on the host."""
    B = c["bytes"].shape[0]
    _, My, Hy, Wy = c["shape_y"]
    _, Nz, Hz, Wz = c["shape_z"]
    dev = c["bytes"].device
    K = c["segments"]
    if K > 1:                                                          # DSIC3
        out = torch.empty(_HEAD.size + _SEGS.size + (_REC.size + 4 * K) * B + B * (c["cap_z"] + K * c["cap_y"]),
                          dtype=torch.uint8, device=dev)
        ws = torch.empty((1 + K) * B + 3, dtype=torch.int64, device=dev)
        _lib.check(_lib.load().dsic_container_pack_seg(_p(c["bytes"]), c["cap_z"], c["cap_y"], K, _p(c["lengths"]),
                                                       _p(c["meta"]), _p(c["err"]), B, tag & 0xFFFFFFFF, My, Hy, Wy,
                                                       Nz, Hz, Wz, _p(ws), _p(out), _stream()), "container_pack_seg")
        nbytes, code = (int(v) for v in ws[:2].cpu())
        return out, nbytes, code
    out = torch.empty(_HEAD.size + _REC.size * B + B * (c["cap_z"] + c["cap_y"]), dtype=torch.uint8, device=dev)
    ws = torch.empty(2 * B + 3, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().dsic_container_pack(_p(c["bytes"]), c["cap_z"], c["cap_y"], _p(c["lengths"]), _p(c["meta"]),
                                               _p(c["err"]), B, tag & 0xFFFFFFFF, My, Hy, Wy, Nz, Hz, Wz, _p(ws),
                                               _p(out), _stream()), "container_pack")
    nbytes, code = (int(v) for v in ws[:2].cpu())
    return out, nbytes, code


@torch.no_grad()
def compress_to_container(model, x, tail=10, Lmax=DEFAULT_LMAX, segments=1) -> bytes:
    """pack_container(custom_compress(model, x, tail, Lmax, segments)), byte for byte, with the container assembled on
    the device: one copy of exactly the container's bytes leaves the GPU."""
    c = _coded_batch(model, x, tail, Lmax, "compress_to_container", pack=True, segments=segments)
    return c["container"][:c["container_bytes"]].cpu().numpy().tobytes()


def _padded_bytes(n):
    """Size of the device copy of n stream bytes: whole 16-byte chunks and at least one spare, so the 16-byte reads of
    the string movers (image_codec.hip load16_any) stay inside the allocation."""
    return (n + 31) // 16 * 16


def _upload_padded(parts, tail, dev):
    """Byte strings, back to back, and behind their padding (16-byte aligned) the numpy array tail, in one host buffer
    and one copy -> (device uint8 [_padded_bytes(total)], total, the device copy of tail as uint8)."""
    total = sum(len(p) for p in parts)
    padded = _padded_bytes(total)
    host = torch.empty(padded + tail.nbytes, dtype=torch.uint8)
    a, off = host.numpy(), 0
    for p in parts:
        a[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
        off += len(p)
    a[padded:] = tail.view(np.uint8).ravel()
    d = host.to(dev)
    return d[:padded], total, d[padded:]


def _decode_selected(model, images, parts, shape_y, shape_z, what, Lmax=None, ride=None, segments=1, seg_lengths=None,
                     residual=None):
    """One decode batch from the strings of n images picked anywhere: images as read_container_head gives them, with
    z_off / y_off counted inside the byte strings `parts` laid back to back; shape_y / shape_z = [n, channels, h, w].
    The strings travel in one padded copy with an int64 control block behind them: descriptors [n][4] (z offset, z
    length, y offset, y length), meta int32 [n][4] (ymin, Ly, zmin, Lz), for segments = K > 1 the int32 [n][K]
    seg_lengths (per image the lengths of its y segments, which lie back to back in its y string), then the int32
    array `ride` (codec's tile numbers).  The device spreads the strings at custom_decompress's strides (_upload_strings) and decodes with Lmax
    (default: _default_lmax over these images).  Returns (g_s's output, not yet clamped; the padded string bytes
    uploaded; the device copy of ride).
    residual (codec's near-lossless streams): residual.decode_spec's dict, whose spans lie in `parts` beside the
    strings; its control words travel behind ride in the same copy, and the tuple gains the decoded q planes."""
    dev = next(model.parameters()).device
    n = len(images)
    rec = np.array(images, dtype=np.int64).reshape(n, 8)
    ride = np.zeros(0, dtype=np.int32) if ride is None else np.asarray(ride, dtype=np.int32)
    nseg = n * segments if segments > 1 else 0
    tail_words = (nseg + ride.size + 1) // 2
    block = np.zeros(6 * n + tail_words, dtype=np.int64)
    block[:4 * n] = rec[:, 4:].ravel()
    meta_np = block[4 * n:6 * n].view(np.int32).reshape(n, 4)
    meta_np[:, 0::2] = rec[:, 0:4:2]
    meta_np[:, 1::2] = rec[:, 1:4:2] - rec[:, 0:4:2] + 1
    if nseg:
        block[6 * n:].view(np.int32)[:nseg] = np.asarray(seg_lengths, dtype=np.int32).reshape(nseg)
    block[6 * n:].view(np.int32)[nseg:nseg + ride.size] = ride
    if residual is not None:
        layer = residual["layer"]                  # the module the spec names: residual or residual16
        block = np.concatenate([block, layer.control_words(residual)])
    d_blob, total, d_block = _upload_padded(parts, block, dev)
    d_block = d_block.view(torch.int64)
    meta = d_block[4 * n:6 * n].view(torch.int32).view(n, 4)
    zmax, ymax = int(rec[:, 5].max()), int(rec[:, 7].max())
    zstride, ystride = max(4, (zmax + 3) // 4 * 4), max(4, (ymax + 3) // 4 * 4)
    zbuf = torch.empty(n * zstride, dtype=torch.uint8, device=dev)
    ybuf = torch.empty(n * ystride, dtype=torch.uint8, device=dev)
    lengths = torch.empty((n, 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().dsic_strings_scatter_select(_p(d_blob), total, _p(d_block), n, max(zmax, ymax), _p(zbuf),
                                                       zstride, _p(ybuf), ystride, _p(lengths), _stream()),
               "strings_scatter_select")
    if Lmax is None:
        Lmax = _default_lmax(model, meta_np)
    tail32 = d_block[6 * n:6 * n + tail_words].view(torch.int32)
    x_hat = _decode_batch(model, shape_y, shape_z, meta, Lmax, (zbuf, zstride, lengths, 2, 0),
                          (ybuf, ystride, lengths, 2, 1), what, segments, tail32[:nseg] if nseg else None)
    if residual is not None:
        q = layer.decode_q(d_blob, total, d_block[6 * n + tail_words:], residual)
        return x_hat, _padded_bytes(total), tail32[nseg:nseg + ride.size], q
    return x_hat, _padded_bytes(total), tail32[nseg:nseg + ride.size]


@torch.no_grad()
def decompress_container(model, blob, Lmax=None):
    """custom_decompress(model, unpack_container(blob)), bit for bit: every image of the blob through
    _decode_selected.  The host reads the header and the 24-byte records; the strings are uploaded once and moved
    into the decoder's buffers on the device."""
    blob = bytes(blob)
    tag, shape_y, shape_z, images, K, seg = _blob_head(blob)
    _refuse_tag(tag, "decompress_container")
    body = images[0][4]                                                # the strings follow the records
    images = [r[:4] + (r[4] - body, r[5], r[6] - body, r[7]) for r in images]
    return _decode_selected(model, images, [memoryview(blob)[body:]], shape_y, shape_z, "decompress_container",
                            Lmax, segments=K, seg_lengths=seg)[0].clamp(0, 1)
