"""Scenes in closed form, for images too large to build or keep on the host (no tests here, nothing of dsic_amd).

A sample is a pure integer function of its coordinates (y, x, c), computed in int64 without ever leaving 63 bits, so
NumPy on the host and torch on a device give the same bytes and no large array has to exist on the host: the device
image is filled block by block, and the host evaluates any list of rows on demand.

  h0 = (y * KY) ^ (x * KX) ^ (c * KC) ^ SEED          under 2^45 for coordinates under 2^17
  h  = mix(h0 & M32), mix(v) = three rounds of v ^= v >> s; v = (v * odd constant) & M32   (products under 2^63)
  uint8:   h & 0xFF          uint16: U16_LO + h % U16_SPAN, inside [U16_LO, U16_LO + U16_SPAN)
  float32: (h & 0xFFFFFF) / 2^24, a 24-bit integer scaled by a power of two: exact in both libraries

uint16 samples keep away from the ends of the range so that a scene can plant its band minimum and maximum at chosen
pixels (Scene.plants); every plant is part of the closed form, on the device and on the host alike.

Validity (uint8 [H][W], 0 = invalid) is a second formula: 32 x 32 blocks that are invalid as a whole (one in eight),
blocks that are valid as a whole (one in eight), and in the others runs of zeros along x whose length and phase depend
on the row.  Valid pixels carry a hashed byte in 1 .. 255, so a wrapped read differs in value as well as in class.

The nodata variant (Scene.nodata = v) plants v in every channel over rectangles: whole 32 x 32 blocks (one in eight),
and a lattice of 20 x 30 rectangles that cut blocks in part; one block in eight holds no nodata pixel at all (its
samples that happen to equal v in every channel are moved off it), so tiles are empty, partial and full in every band.
"""
import numpy as np

KY, KX, KC, SEED = 73856093, 19349663, 83492791, 0x5BD1E995
M32 = 0xFFFFFFFF
MIX = ((15, 0x2C1B3C6D), (12, 0x297A2D39), (15, 0x1B873593))
U16_LO, U16_SPAN = 256, 65024
BLOCK_BYTES = 64 << 20                         # the int64 temporaries of one evaluated block on the device
CONSTANTS = {"KY": KY, "KX": KX, "KC": KC, "SEED": SEED, "MIX": [list(m) for m in MIX], "U16_LO": U16_LO,
             "U16_SPAN": U16_SPAN}             # what a recorded fixture names to say which pattern it was made from

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def mix(v):
    """int64 array (either library) -> int64 in [0, 2^32)"""
    v = v & M32
    for s, k in MIX:
        v = v ^ (v >> s)
        v = (v * k) & M32
    return v ^ (v >> 16)


def value(y, x, c, kind):
    """The sample at (y, x, c): broadcastable int64 arrays of NumPy or torch -> int64 (u8, u16) or the 24-bit
    numerator of the float32 sample (f32)."""
    h = mix((y * KY) ^ (x * KX) ^ (c * KC) ^ SEED)
    if kind == "u8":
        return h & 0xFF
    if kind == "u16":
        return U16_LO + h % U16_SPAN
    assert kind == "f32"
    return h & 0xFFFFFF


def block_class(y, x, salt):
    """0 .. 7 per 32 x 32 block"""
    return mix(((y >> 5) * KX) ^ ((x >> 5) * KY) ^ salt) & 7


def validity(y, x):
    """int64: 0 = invalid, else a byte in 1 .. 255"""
    cls = block_class(y, x, 0x1234567)
    run = 3 + (mix(y * KC + 17) & 31)                                    # zeros come in runs of 3 .. 34 along x
    in_run = ((x + (mix(y * KX + 5) & 63)) % (2 * run + 7)) < run
    byte = 1 + mix((y * KX) ^ (x * KY) ^ 0x7777) % 255
    zero = (cls == 0) | ((cls != 1) & in_run)
    return byte * (1 - zero * 1)


def nodata_class(y, x):
    """0 = nodata here, 1 = never nodata here, 2 = the samples decide"""
    cls = block_class(y, x, 0x2468ACE)
    rect = ((y % 97) < 20) & ((x % 113) < 30)
    planted = (cls == 0) | ((cls != 1) & rect)
    return (1 - planted * 1) * (1 + (cls != 1) * 1)


class _Np:
    """the array namespace of NumPy, as the scenes use it"""
    int64 = np.int64

    @staticmethod
    def arange(a, b):
        return np.arange(a, b, dtype=np.int64)

    @staticmethod
    def asarray(v):
        return np.asarray(v, dtype=np.int64)

    @staticmethod
    def cast(v, kind):
        if kind == "f32":
            return v.astype(np.float32) / np.float32(1 << 24)
        return v.astype(DTYPES[kind])

    @staticmethod
    def where(c, a, b):
        return np.where(c, a, b)


class _Torch:
    """the same of torch, on a device; uint16 samples are held as int16 tensors of the same bits"""

    def __init__(self, device):
        import torch
        self.t, self.device = torch, device

    def arange(self, a, b):
        return self.t.arange(a, b, dtype=self.t.int64, device=self.device)

    def asarray(self, v):
        return self.t.as_tensor(np.asarray(v, dtype=np.int64), device=self.device)

    def cast(self, v, kind):
        t = self.t
        if kind == "f32":
            return v.to(t.float32) / float(1 << 24)
        if kind == "u16":                                                    # the same 16 bits, held as int16
            return ((v + 32768) % 65536 - 32768).to(t.int16)
        return v.to(t.uint8)

    def where(self, c, a, b):
        return self.t.where(c, a, b)


NP = _Np()


def torch_namespace(device):
    return _Torch(device)


class Scene:
    """kind u8 / u16 (layout HWC) or f32 (layout CHW) of H x W x C.  nodata: the planted value or None.  plants:
    ((y, x, c, value), ...) single samples that replace the formula's."""

    def __init__(self, name, kind, H, W, C, valid=False, nodata=None, plants=()):
        self.name, self.kind, self.H, self.W, self.C = name, kind, int(H), int(W), int(C)
        self.valid, self.nodata, self.plants = bool(valid), nodata, tuple(plants)
        self.layout = "chw" if kind == "f32" else "hwc"
        self.item = np.dtype(DTYPES[kind]).itemsize
        self.dtype = np.dtype(DTYPES[kind])

    @property
    def elements(self):
        return self.H * self.W * self.C

    @property
    def nbytes(self):
        return self.elements * self.item

    def shape(self, rows=None):
        h = self.H if rows is None else rows
        return (self.C, h, self.W) if self.layout == "chw" else (h, self.W, self.C)

    def samples(self, xp, y, x, c):
        """The formula with the planted nodata value, without the single plants, at broadcastable coordinates -> int64:
        what rows() evaluates, and what a read at any other offset of the image would find."""
        v = value(y, x, c, self.kind)
        if self.nodata is not None:
            cls = nodata_class(y, x)
            # a pixel that must not be nodata gets channel 0 moved off the value; it costs nothing elsewhere
            off = (self.nodata + 1) % (256 if self.kind == "u8" else 65536)
            v = xp.where(cls == 0, v * 0 + self.nodata, xp.where((cls == 1) & (c == 0) & (v == self.nodata), v * 0 + off, v))
        return v

    def rows(self, xp, ys):
        """The samples of the rows `ys` (any order, repeats allowed): [len(ys)][W][C], or [C][len(ys)][W] for CHW."""
        ys = np.asarray(ys, dtype=np.int64)
        y, x, c = xp.asarray(ys), xp.arange(0, self.W), xp.arange(0, self.C)
        if self.layout == "chw":
            y, x, c = y[None, :, None], x[None, None, :], c[:, None, None]
        else:
            y, x, c = y[:, None, None], x[None, :, None], c[None, None, :]
        v = self.samples(xp, y, x, c)
        for py, px, pc, pv in self.plants:
            for k in np.flatnonzero(ys == py):
                if self.layout == "chw":
                    v[pc, int(k), px] = pv
                else:
                    v[int(k), px, pc] = pv
        return xp.cast(v, self.kind)

    def valid_rows(self, xp, ys):
        """uint8 [len(ys)][W]"""
        y, x = xp.asarray(np.asarray(ys, dtype=np.int64))[:, None], xp.arange(0, self.W)[None, :]
        return xp.cast(validity(y, x), "u8")

    def band(self, y0, y1):
        """rows [y0, y1) on the host"""
        return self.rows(NP, np.arange(y0, y1))

    def valid_band(self, y0, y1):
        return self.valid_rows(NP, np.arange(y0, y1))

    def block_rows(self):
        """rows of one evaluated block on the device: its int64 temporaries stay within BLOCK_BYTES"""
        return max(1, BLOCK_BYTES // (8 * self.W * self.C))

    def fill(self, xp, image, valid=None):
        """Fills the device tensors image (shape()) and valid ([H][W]) block by block."""
        step = self.block_rows()
        for y0 in range(0, self.H, step):
            ys = np.arange(y0, min(y0 + step, self.H))
            blk = self.rows(xp, ys)
            if self.layout == "chw":
                image[:, y0:y0 + len(ys)] = blk
            else:
                image[y0:y0 + len(ys)] = blk
        if valid is not None:
            vstep = max(1, BLOCK_BYTES // (8 * self.W))
            for y0 in range(0, self.H, vstep):
                ys = np.arange(y0, min(y0 + vstep, self.H))
                valid[y0:y0 + len(ys)] = self.valid_rows(xp, ys)

    # ---- flat offsets ---------------------------------------------------------------------------------------------
    def coords(self, e):
        """flat element numbers -> (y, x, c)"""
        e = np.asarray(e, dtype=np.int64)
        if self.layout == "chw":
            c, r = np.divmod(e, self.H * self.W)
            y, x = np.divmod(r, self.W)
        else:
            p, c = np.divmod(e, self.C)
            y, x = np.divmod(p, self.W)
        return y, x, c

    def at(self, e):
        """the samples at flat element numbers, on the host, as int64 (the float32 numerator for f32)"""
        y, x, c = self.coords(e)
        assert self.nodata is None and not self.plants
        return value(y, x, c, self.kind)

    def crossings(self):
        """{name: flat element number} of the first element at or past 2^31 / 2^32 elements and bytes inside the image"""
        out = {}
        for name, e in (("2^31 elements", 1 << 31), ("2^32 elements", 1 << 32), ("2^31 bytes", (1 << 31) // self.item),
                        ("2^32 bytes", (1 << 32) // self.item)):
            if e < self.elements:
                out[name] = e
        return out

    def crossing_rows(self):
        """the image rows (HWC) or plane rows (CHW: as (c, y)) that hold a crossing -> sorted row numbers y"""
        return sorted({int(self.coords(e)[0]) for e in self.crossings().values()})


def table(bands=True):
    """The geometries of the large-image tests, the smallest that cross each threshold with rows of ordinary width;
    H and W are no multiples of 16."""
    H16, W16 = 32801, 16401
    u16_plants = tuple((H16 - 5, 7 + c, c, 3 + c) for c in range(4)) + \
        tuple((H16 - 2, W16 - 3 - c, c, 65535 - c) for c in range(4))
    return {
        "u8c3": Scene("u8c3", "u8", 39801, 36001, 3, valid=True, nodata=7),
        "u8c1v": Scene("u8c1v", "u8", 32801, 65537, 1, valid=True),
        "u16c4": Scene("u16c4", "u16", H16, W16, 4, valid=True, plants=u16_plants if bands else ()),
        "f32c3": Scene("f32c3", "f32", 26801, 26801, 3),
        "tiles16_u8": Scene("tiles16_u8", "u8", 8209, 8209, 3, valid=True, nodata=7),
        "tiles16_u16": Scene("tiles16_u16", "u16", 8209, 8209, 3, valid=True, nodata=7),
        # three channels (the uint8 resamplers take no fewer) with pixel 2^31 inside image and validity
        "u8c3v": Scene("u8c3v", "u8", 32801, 65537, 3, valid=True, nodata=7),
        # the masked uint16 halving with a destination past 2^31 bytes: 8.6 GB of image, 1.1 GB of validity
        "halve_valid_u16": Scene("halve_valid_u16", "u16", 92801, 11601, 4, valid=True),
    }
