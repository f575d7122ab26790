"""A torch restatement of include/sesrq_noise.h that runs on the frame's device, in chunks -- TEST INFRASTRUCTURE (not collected).

tests/noise_oracle.py needs 1.5 s for 4 M pixels, so frames of 10^8 .. 10^9 pixels are compared here instead: the same header, written
again in torch, evaluated chunk by chunk (CHUNK_PX pixels: no live tensor of this module exceeds 3 GiB, the rule of tests/geometry.py;
at 2^21 pixels the largest, a float64 (3, chunk) temporary, has 48 MiB).  tests/test_noise_device.py pins every stage to
tests/noise_oracle.py, on the CPU and on the device, before tests/test_noise_limits.py relies on it.

  words     Philox4x32-10 in int64.  A product c M of two 32-bit values wraps in signed 64 bits but keeps the bits of the unsigned
            product: (p >> 32) & 0xFFFFFFFF and p & 0xFFFFFFFF are its two halves (the arithmetic shift's sign bits are masked off).
  deviates  float64, as noise_oracle.deviates: compared with the device's fp32 deviates at a tolerance the caller gives (T_Z).
  combine, clamp, quantise: bit for bit, from the DEVICE'S deviates, as noise_oracle.frame.  Every fp32 step is the float64 operation
            followed by .float(): for +, x, / and sqrt of fp32 operands that IS the correctly rounded fp32 operation (double rounding
            is innocuous at 53 >= 2 * 24 + 2 bits), whatever torch's fp32 kernels were compiled to do, subnormal results included.
            rint (torch.round: half to even) and the clamps are exact.  The clamp is fmin(fmax(y, 0), 1): a NaN y gives 0, as the
            header says.

Only counts leave the device, with the first few mismatching (n, c, y, x) and what was there.

Frames are described by a callable codes(n0, n1, r0, r1, x0, x1) -> integer tensor (n1 - n0, r1 - r0, x1 - x0) on the device: Dense
wraps a tensor that exists, Tiled repeats a small (F, PY, PX) block (frame n is block n mod F), so that a frame of 10^9 pixels needs
no codes tensor.  build_raw packs such a frame into the rows sesrq_noise_unpack reads, on the device, band by band."""
import numpy as np

F32 = np.float32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
U64 = (1 << 64) - 1
Z_MAX = float(np.sqrt(48 * np.log(2.0)))
SITE = {"rggb": ((0, 1), (1, 2)), "grbg": ((1, 0), (2, 1)), "gbrg": ((1, 2), (0, 1)), "bggr": ((2, 1), (1, 0))}     # [y & 1][x & 1]
CHUNK_PX = 1 << 21
FIRST = 4                         # mismatching coordinates a report keeps per output


def _i64(values, dev):
    """Unsigned 32-bit python ints -> an int64 tensor."""
    import torch
    return torch.from_numpy(np.asarray(values, np.int64)).to(dev)


def philox(c, key):
    """Philox4x32-10.  c: four int64 tensors holding 32-bit values (broadcast against each other), key: two ints."""
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = c[0] * M0, c[2] * M1
        c = [((p1 >> 32) & MASK) ^ c[1] ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c[3] ^ k1, p0 & MASK]
    return c


def words(seed, frames, r0, r1, x0, x1, dev):
    """(w0, w1, w2, w3), each (len(frames), r1 - r0, x1 - x0) int64, of pixels (r0 .. r1 - 1, x0 .. x1 - 1) of the frames whose global
    numbers `frames` lists."""
    import torch
    seed = int(seed) & U64
    f = [int(v) & U64 for v in frames]
    x = torch.arange(x0, x1, dtype=torch.int64, device=dev).view(1, 1, -1)
    y = torch.arange(r0, r1, dtype=torch.int64, device=dev).view(1, -1, 1)
    lo, hi = _i64([v & MASK for v in f], dev).view(-1, 1, 1), _i64([v >> 32 for v in f], dev).view(-1, 1, 1)
    return [w.expand(len(f), r1 - r0, x1 - x0) for w in philox([x, y, lo, hi], (seed & MASK, seed >> 32))]


def deviates(w):
    """(n, 3, R, W) float64 from the four words."""
    import torch
    ua, ub = ((w[0] >> 9).double() + 0.5) * 2.0 ** -23, ((w[2] >> 9).double() + 0.5) * 2.0 ** -23
    ta, tb = 2.0 * np.pi * ((w[1] >> 8).double() * 2.0 ** -24), 2.0 * np.pi * ((w[3] >> 8).double() * 2.0 ** -24)
    ra, rb = torch.sqrt(-2.0 * torch.log(ua)), torch.sqrt(-2.0 * torch.log(ub))
    return torch.stack([ra * torch.cos(ta), ra * torch.sin(ta), rb * torch.cos(tb)], 1)


def clean(codes, cfa, black, white, r0, x0):
    """(n, R, W) codes whose first pixel is (r0, x0) of its frame -> the clean (n, 3, R, W) fp32 frame: fl32(d) / fl32(white - black)
    at the site channel, 0 elsewhere."""
    import torch
    dev = codes.device
    d = codes.to(torch.int64).clamp(black, white) - black
    x = (d.double() / float(white - black)).float()
    t = torch.tensor(SITE[cfa], dtype=torch.int64, device=dev)
    yy = (torch.arange(r0, r0 + codes.shape[1], device=dev) & 1).view(-1, 1)
    xx = (torch.arange(x0, x0 + codes.shape[2], device=dev) & 1).view(1, -1)
    site = t[yy, xx]                                                                          # (R, W)
    ch = torch.arange(3, device=dev).view(1, 3, 1, 1)
    return torch.where(site.view(1, 1, *site.shape) == ch, x.unsqueeze(1), torch.zeros((), dtype=torch.float32, device=dev))


def combine(x, shot, read, z):
    """spread = min(max(x + sqrt(x * shot + read) * z, 0), 1), every step one correctly rounded fp32 operation.  x, z: fp32 tensors;
    shot, read: fp32 tensors that broadcast against them."""
    import torch
    v = ((x.double() * shot.double()).float().double() + read.double()).float()
    s = torch.sqrt(v.double()).float()
    y = (x.double() + (s.double() * z.double()).float().double()).float()
    zero, one = torch.zeros((), dtype=torch.float32, device=x.device), torch.ones((), dtype=torch.float32, device=x.device)
    return torch.fmin(torch.fmax(y, zero), one)


def quantise(sp, s0, z0, exact_div):
    """q0 = clamp8(rint(fl(fl(sp / s0) + z0))); exact_div 2: sp * fl(1 / s0)."""
    import torch
    s0 = F32(s0)
    t = (sp.double() * float(F32(1) / s0)).float() if exact_div == 2 else (sp.double() / float(s0)).float()
    return torch.round((t.double() + float(z0)).float()).clamp(-128, 127).to(torch.int8)


def pack(codes, packing):
    """(..., W) integer codes -> (..., row bytes) uint8 as include/sesrq_sensor.h lays them out: little-endian uint16; MIPI RAW10
    (four pixels: their high 8 bits, then one byte of the four low pairs, pixel 0 lowest); RAW12 (two pixels: their high 8 bits, then
    one byte of the two low nibbles, pixel 0 lowest)."""
    import torch
    c = codes.to(torch.int64)
    lead = tuple(c.shape[:-1])
    if packing == "u16":
        out = torch.stack([c & 255, c >> 8], -1)
    elif packing == "raw10":
        p = c.reshape(*lead, -1, 4)
        low = (p[..., 3] & 3) << 6 | (p[..., 2] & 3) << 4 | (p[..., 1] & 3) << 2 | (p[..., 0] & 3)
        out = torch.cat([p >> 2, low.unsqueeze(-1)], -1)
    else:
        p = c.reshape(*lead, -1, 2)
        out = torch.cat([p >> 4, ((p[..., 1] & 15) << 4 | (p[..., 0] & 15)).unsqueeze(-1)], -1)
    return out.reshape(*lead, -1).to(torch.uint8)


def row_bytes(packing, W):
    return {"u16": 2 * W, "raw10": W // 4 * 5, "raw12": W // 2 * 3}[packing]


class Dense:
    """A frame whose (N, H, W) codes exist as a tensor."""

    def __init__(self, codes):
        self.codes = codes

    def __call__(self, n0, n1, r0, r1, x0, x1):
        return self.codes[n0:n1, r0:r1, x0:x1]


class Tiled:
    """codes[n, y, x] = tile[n mod F, y mod PY, x mod PX] of a small (F, PY, PX) integer tile on the device.  PY and PX even keep the
    Bayer phase."""

    def __init__(self, tile):
        self.tile = tile
        assert tile.shape[1] % 2 == 0 and tile.shape[2] % 2 == 0

    def __call__(self, n0, n1, r0, r1, x0, x1):
        import torch
        F, PY, PX = self.tile.shape
        dev = self.tile.device
        n = torch.arange(n0, n1, device=dev) % F
        y = torch.arange(r0, r1, device=dev) % PY
        x = torch.arange(x0, x1, device=dev) % PX
        return self.tile[n.view(-1, 1, 1), y.view(1, -1, 1), x.view(1, 1, -1)]


def chunks(N, H, W, px=None):
    """(n0, n1, r0, r1, x0, x1) boxes of at most `px` pixels that tile (N, H, W): whole frames, else whole rows, else an even number of
    columns of one row."""
    px = CHUNK_PX if px is None else px
    assert px % 2 == 0
    if H * W <= px:
        step = max(1, px // (H * W))
        return [(n, min(N, n + step), 0, H, 0, W) for n in range(0, N, step)]
    if W <= px:
        step = max(1, px // W)
        return [(n, n + 1, r, min(H, r + step), 0, W) for n in range(N) for r in range(0, H, step)]
    return [(n, n + 1, r, r + 1, x, min(W, x + px)) for n in range(N) for r in range(H) for x in range(0, W, px)]


def build_raw(codes, N, H, W, packing, stride=None, pad=0xEE, dev=None):
    """The (N, H, stride) uint8 rows of the frame, packed on the device box by box; stride padding holds `pad`."""
    import torch
    nb = row_bytes(packing, W)
    stride = nb if stride is None else stride
    group = {"u16": (1, 2), "raw10": (4, 5), "raw12": (2, 3)}[packing]
    raw = torch.empty((N, H, stride), dtype=torch.uint8, device=dev)
    if stride > nb:
        raw[:, :, nb:] = pad
    for n0, n1, r0, r1, x0, x1 in chunks(N, H, W, CHUNK_PX - CHUNK_PX % 4):
        raw[n0:n1, r0:r1, x0 // group[0] * group[1]:x1 // group[0] * group[1]] = pack(codes(n0, n1, r0, r1, x0, x1), packing)
    return raw


class Report:
    """What one comparison found: counts per output, the first mismatches, and the deviates' largest error."""

    def __init__(self):
        self.bad = {"z": 0, "z_range": 0, "spread": 0, "q0": 0}
        self.first = {k: [] for k in self.bad}
        self.compared = {k: 0 for k in self.bad}
        self.z_err, self.z_at, self.z_there = 0.0, None, 0.0

    def note(self, key, mask, box, got, want):
        import torch
        self.compared[key] += mask.numel()
        k = int(torch.count_nonzero(mask))
        if not k:
            return
        self.bad[key] += k
        if len(self.first[key]) < FIRST:
            idx = mask.reshape(-1).nonzero()[:FIRST - len(self.first[key])].flatten().cpu().numpy()
            for i in idx:
                j = tuple(int(v) for v in np.unravel_index(int(i), tuple(mask.shape)))
                at = (j[0] + box[0], j[1], j[2] + box[2], j[3] + box[4])
                self.first[key].append((at, got[j].item(), want[j].item() if want is not None else None))

    def clean(self, what=""):
        assert not any(self.bad.values()), f"{what}: {self}"

    def __repr__(self):
        parts = [f"{k}: {self.bad[k]} of {self.compared[k]} differ, first (at (n, c, y, x), got, want) {self.first[k]}"
                 for k in self.bad if self.bad[k]]
        return "; ".join(parts) or f"no mismatch in {self.compared}"


def compare(codes, N, H, W, z, *, seed, frame0, tol, cfa=None, black=0, white=4095, levels=None, s0=None, z0=None, exact_div=0,
            spread=None, q0=None, check_z=True, boxes=None):
    """Every element of the device outputs of one call against the header, box by box.

    z: the device's (N, 3, H, W) fp32 deviates of (seed, frame0): compared with the float64 deviates at `tol` and with Z_MAX
    (check_z), and the input of the exact part.  spread / q0: outputs of sesrq_noise_unpack on the frame `codes` describes (either may
    be None), compared bit for bit with combine / quantise of z.  levels: (shot, read), or an (N, 2) fp32 array of per-frame pairs.
    boxes: a subset of chunks(N, H, W) (default: all of them)."""
    import torch
    dev = z.device
    rep = Report()
    lv = None
    if spread is not None or q0 is not None:
        lv = torch.from_numpy(np.array(np.broadcast_to(np.asarray(levels, F32), (N, 2)), order="C", copy=True)).to(dev)
    for box in (chunks(N, H, W) if boxes is None else boxes):
        n0, n1, r0, r1, x0, x1 = box
        zd = z[n0:n1, :, r0:r1, x0:x1]
        if check_z:
            want = deviates(words(seed, [(int(frame0) + n) & U64 for n in range(n0, n1)], r0, r1, x0, x1, dev))
            err = (zd.double() - want).abs()
            rep.note("z", ~(err <= tol), box, zd, want)                  # a NaN is over the tolerance
            rep.note("z_range", ~(zd.double().abs() <= Z_MAX), box, zd, None)
            m = float(err.max())
            if m > rep.z_err:
                j = tuple(int(v) for v in np.unravel_index(int(err.argmax()), tuple(err.shape)))
                rep.z_err, rep.z_at, rep.z_there = m, (j[0] + n0, j[1], j[2] + r0, j[3] + x0), float(zd[j])
            del want, err
        if lv is not None:
            x = clean(codes(*box), cfa, black, white, r0, x0)
            sp = combine(x, lv[n0:n1, 0].view(-1, 1, 1, 1), lv[n0:n1, 1].view(-1, 1, 1, 1), zd)
            if spread is not None:
                got = spread[n0:n1, :, r0:r1, x0:x1]
                rep.note("spread", got.view(torch.int32) != sp.view(torch.int32), box, got, sp)
            if q0 is not None:
                wq = quantise(sp, s0, z0, exact_div)
                got = q0[n0:n1, :, r0:r1, x0:x1]
                rep.note("q0", got != wq, box, got, wq)
            del x, sp
    return rep
