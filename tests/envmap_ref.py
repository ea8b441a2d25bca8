"""Numpy restatement of include/bevyray_amd.h "reflection probes": texel directions, the resolve, the box level, the tap tables and the
filter rule.  Every function takes the dtype it computes in: np.float32 restates the library operation by operation (every numpy f32
operation is separately rounded, like the library's under -ffp-contract=off) and must agree with it to the bit; np.float64 is the same
rule in double precision, the yardstick the f32 tolerances are measured against.  The tap tables are float64 by definition (rounded
once to f32)."""
import numpy as np

SEED_STEP = 0x9E3779B9
TAPS_GGX, TAPS_COSINE = 0, 1
# raw = (sx * [1|u|v] ...) per face: written out, as in the header
FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")


def level_offsets(size, levels):
    offs = [0]
    for l in range(levels):
        offs.append(offs[-1] + 6 * (size >> l) ** 2)
    return offs


def directions(size, dt=np.float32):
    """(6, size, size, 3): d of texel (face, y, x)."""
    f = dt
    idx = np.arange(size, dtype=np.uint32)
    c = (f(1) * (2 * idx + 1).astype(dt)) / f(size) - f(1)
    u = np.broadcast_to(c[None, :], (size, size)).astype(dt)
    v = np.broadcast_to(c[:, None], (size, size)).astype(dt)
    one = np.ones((size, size), dt)
    raw = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)]
    out = np.zeros((6, size, size, 3), dt)
    for face, (x, y, z) in enumerate(raw):
        ln = np.sqrt((x * x + y * y) + z * z)
        out[face, ..., 0], out[face, ..., 1], out[face, ..., 2] = x / ln, y / ln, z / ln
    return out


def seeds(seed, size):
    return ((np.arange(6 * size * size, dtype=np.uint64) * SEED_STEP + seed) & 0xFFFFFFFF).astype(np.uint32)


def resolve(rgb, status, dt=np.float32):
    """rgb (n, 3) of the radiance results and their status words -> (n, 4) texels."""
    rgb = np.asarray(rgb).astype(dt)
    out = np.zeros((len(rgb), 4), dt)
    with np.errstate(all="ignore"):
        out[:, :3] = rgb * rgb
    out[:, 3] = np.where((np.asarray(status) & 1) != 0, dt(1), dt(0))
    return out


def downsample(src, dt=np.float32):
    """(6, S, S, 4) -> (6, S / 2, S / 2, 4)."""
    s = np.asarray(src).astype(dt)
    with np.errstate(all="ignore"):
        return ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])) * dt(0.25)


def radical_inverse(i):
    r = 0
    for b in range(32):
        r |= ((i >> b) & 1) << (31 - b)
    return r / 4294967296.0


def taps64(kind, roughness, n):
    """The table in float64, (n, 4); roughness is the f32 argument.  Rounded once to f32 it is the library's table up to libm."""
    out = np.zeros((n, 4), np.float64)
    for i in range(n):
        xi1, xi2 = (i + 0.5) / n, radical_inverse(i)
        phi = 2.0 * np.pi * xi1
        cp, sp = np.cos(phi), np.sin(phi)
        if kind == TAPS_GGX:
            a = float(np.float32(roughness)) ** 2
            ct = np.sqrt((1.0 - xi2) / (1.0 + (a * a - 1.0) * xi2))
            st = np.sqrt(max(0.0, 1.0 - ct * ct))
            h = (st * cp, st * sp, ct)
            l = (2.0 * h[2] * h[0], 2.0 * h[2] * h[1], 2.0 * h[2] * h[2] - 1.0)
            w = max(l[2], 0.0)
        else:
            r = np.sqrt(xi2)
            l = (r * cp, r * sp, np.sqrt(1.0 - xi2))
            w = 1.0
        out[i] = (l[0], l[1], l[2], w)
    return out


def _axis(u, size, dt):
    f = dt
    hi = f(size - 1)
    px = ((u + f(1)) * f(0.5)) * f(size) - f(0.5)
    clamped = (px < 0) | (px > hi)
    px = np.where(px > 0, px, f(0)).astype(dt)          # (a NaN becomes 0)
    px = np.where(px < hi, px, hi).astype(dt)
    cell = np.floor(px).astype(np.int64)
    i0 = np.minimum(cell, max(size, 2) - 2)
    i1 = np.minimum(i0 + 1, size - 1)
    g = px - i0.astype(dt)
    return i0, i1, g.astype(dt), clamped


def filter_cube(src, taps, dst_size, dt=np.float32, info=None):
    """The filter rule: (6, S, S, 4) cube and (n, 4) table -> (6, dst_size, dst_size, 4).  info (a dict): which faces the taps reached,
    whether the clamp at a face edge was taken, and which branches of the frame were."""
    f = dt
    src = np.asarray(src).astype(dt)
    taps = np.asarray(taps).astype(dt).reshape(-1, 4)
    S = src.shape[1]
    N = directions(dst_size, dt).reshape(-1, 3)
    n = len(N)
    up_z = np.abs(N[:, 2]) < f(0.999)
    zero = np.zeros(n, dt)
    t = np.where(up_z[:, None], np.stack([-N[:, 1], N[:, 0], zero], 1), np.stack([zero, -N[:, 2], N[:, 1]], 1)).astype(dt)
    tl = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
    T = (t / tl[:, None]).astype(dt)
    B = np.stack([N[:, 1] * T[:, 2] - N[:, 2] * T[:, 1], N[:, 2] * T[:, 0] - N[:, 0] * T[:, 2], N[:, 0] * T[:, 1] - N[:, 1] * T[:, 0]], 1).astype(dt)
    acc = np.zeros((n, 4), dt)
    sw = np.zeros(n, dt)
    faces_seen, clamp_seen = set(), False
    flat = src.reshape(6 * S * S, 4)
    with np.errstate(all="ignore"):
        for k in range(len(taps)):
            lx, ly, lz, w = taps[k]
            if w <= 0:                                  # (a NaN weight is kept)
                continue
            L = ((lx * T + ly * B) + lz * N).astype(dt)
            ax, ay, az = np.abs(L[:, 0]), np.abs(L[:, 1]), np.abs(L[:, 2])
            isx = (ax >= ay) & (ax >= az)
            isy = ~isx & (ay >= az)
            isz = ~isx & ~isy
            negx, negy, negz = L[:, 0] < 0, L[:, 1] < 0, L[:, 2] < 0
            face = np.where(isx, np.where(negx, 1, 0), np.where(isy, np.where(negy, 3, 2), np.where(negz, 5, 4)))
            ma = np.where(isx, ax, np.where(isy, ay, az)).astype(dt)
            sc = np.where(isx, np.where(negx, L[:, 2], -L[:, 2]), np.where(isy, L[:, 0], np.where(negz, -L[:, 0], L[:, 0]))).astype(dt)
            tc = np.where(isy, np.where(negy, -L[:, 2], L[:, 2]), -L[:, 1]).astype(dt)
            x0, x1, gx, cx = _axis(sc / ma, S, dt)
            y0, y1, gy, cy = _axis(tc / ma, S, dt)
            faces_seen |= set(np.unique(face).tolist())
            clamp_seen |= bool(np.any(cx | cy))
            base = face * S
            c00, c01 = flat[(base + y0) * S + x0], flat[(base + y0) * S + x1]
            c10, c11 = flat[(base + y1) * S + x0], flat[(base + y1) * S + x1]
            hx, hy = (f(1) - gx)[:, None], (f(1) - gy)[:, None]
            gx, gy = gx[:, None], gy[:, None]
            c = (c00 * hx + c01 * gx) * hy + (c10 * hx + c11 * gx) * gy
            acc = (acc + w * c).astype(dt)
            sw = (sw + w).astype(dt)
        out = np.where((sw > 0)[:, None], acc / sw[:, None], f(0)).astype(dt)
    if info is not None:
        info.update(faces=faces_seen, clamped=clamp_seen, up_z=bool(np.any(up_z)), up_x=bool(np.any(~up_z)))
    return out.reshape(6, dst_size, dst_size, 4)


def level_roughness(l, levels):
    return np.float32(l) / np.float32(levels - 1)


def chain(level0, levels, tables, dt=np.float32):
    """level0 (6, S, S, 4) and the tables of the levels 1 .. levels - 1 -> the concatenated (n, 4) chain."""
    out = [np.asarray(level0).astype(dt).reshape(-1, 4)]
    box = np.asarray(level0)
    for l in range(1, levels):
        box = downsample(box, dt)
        out.append(filter_cube(box, tables[l - 1], box.shape[1], dt).reshape(-1, 4))
    return np.concatenate(out)
