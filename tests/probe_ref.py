"""Reference side of tests/test_probes.py: the rule of light probes (DESIGN.md "Light probes") restated in numpy.

Directions (float64, rounded to f32 at the end), N in [1, 65536], k = 0 .. N-1:
    y = 1 - (2k+1)/N;  r = sqrt(max(0, 1 - y*y));  phi = 2 pi frac(k (sqrt(5)-1)/2);  d_k = (f32(r cos phi), f32(y), f32(r sin phi))
`directions64` is that formula; the tests that compare bitwise take the table from the library's export instead (brt.probe_directions),
so that no libm difference reaches them.

Rays: entry k of probe {position, seed} is the radiance entry {position, seed + k * 0x9E3779B9 (mod 2^32), d_k, user = k}, traced with
samples = 1.  Lists are probe-major: entry k of probe p is record p * N + k.

Projection (`project`): f32, every operation separately rounded.  L_k = rgb_k * rgb_k.  Lane l of 64 sums its terms k = l, l + 64, ...
in order from +0.0; then for off = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l + off] for l < off; lane 0 holds the sum.
    SH9:  c[j][ch] = (12.566371f / f32(N)) * sum_k (Y_j(d_k) * L_k[ch]) with the basis of `sh9_basis`
    cube: faces +X, -X, +Y, -Y, +Z, -Z; m = c if c > 0 else 0 for c = +-component; m2 = m * m;
          value = (sum_k m2 * L_k[ch]) / (sum_k m2), 0 where the denominator is 0; words 18..26 are 0
Record: coeff[27], hits (entries with the HIT bit), status (entry 0's INVALID / OUT_OF_REACH bits), n_dirs, basis, 0.  A probe whose
status is not 0 has all coefficients 0 and hits 0."""
import numpy as np

import bevyray_amd as brt

F32 = np.float32
SEED_STEP = 0x9E3779B9
SH9, CUBE = brt.PROBE_SH9, brt.PROBE_AMBIENT_CUBE
REFUSED = brt.QUERY_STATUS_INVALID | brt.QUERY_STATUS_OUT_OF_REACH
SH_A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def directions64(n):
    """The direction formula in numpy float64 -> (n, 3) float64 (not rounded)."""
    k = np.arange(n, dtype=np.float64)
    y = 1.0 - (2.0 * k + 1.0) / float(n)
    r = np.sqrt(np.maximum(0.0, 1.0 - y * y))
    t = k * ((np.sqrt(5.0) - 1.0) / 2.0)
    phi = 2.0 * np.pi * (t - np.floor(t))
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1)


def make_rays(probes, dirs):
    """The probe-major list of RADIANCE_RAY_DTYPE entries of `probes` (PROBE_DTYPE) for the f32 table `dirs`; the probes' words are copied
    as bits."""
    probes = np.ascontiguousarray(probes, brt.PROBE_DTYPE).reshape(-1)
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    p, n = len(probes), len(dirs)
    words = np.zeros((p, n, 8), np.uint32)
    words[:, :, 0:3] = probes["position"].view(np.uint32).reshape(p, 1, 3)
    k = np.arange(n, dtype=np.uint64)
    words[:, :, 3] = ((probes["seed"].astype(np.uint64)[:, None] + k[None, :] * np.uint64(SEED_STEP)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words[:, :, 4:7] = dirs.view(np.uint32)[None, :, :]
    words[:, :, 7] = k.astype(np.uint32)[None, :]
    return words.reshape(p * n, 8).view(brt.RADIANCE_RAY_DTYPE).reshape(p * n)


def sh9_basis(d):
    """Y_0..8 on the f32 components of d (n, 3) -> (n, 9) f32, each operation rounded, in the kernels' order."""
    d = np.asarray(d, F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    a, b, c2, c6, c8 = F32(0.488603), F32(1.092548), F32(0.282095), F32(0.315392), F32(0.546274)
    Y = np.empty((len(d), 9), F32)
    Y[:, 0] = c2
    Y[:, 1] = a * y
    Y[:, 2] = a * z
    Y[:, 3] = a * x
    Y[:, 4] = (b * x) * y
    Y[:, 5] = (b * y) * z
    Y[:, 6] = c6 * (((F32(3.0) * z) * z) - F32(1.0))
    Y[:, 7] = (b * x) * z
    Y[:, 8] = c8 * ((x * x) - (y * y))
    return Y


def cube_weights(d):
    """m2 per face (+X, -X, +Y, -Y, +Z, -Z) -> (n, 6) f32."""
    d = np.asarray(d, F32).reshape(-1, 3)
    c = np.stack([d[:, 0], -d[:, 0], d[:, 1], -d[:, 1], d[:, 2], -d[:, 2]], axis=1)
    m = np.where(c > 0, c, F32(0.0)).astype(F32)
    return (m * m).astype(F32)


def _wave_sum(terms):
    """terms (P, N, A) f32 -> (P, A): the lane-strided accumulation and the six-step tree."""
    p, n, a = terms.shape
    rounds = -(-n // 64)
    with np.errstate(all="ignore"):
        acc = np.zeros((p, 64, a), F32)
        for i in range(rounds):
            chunk = terms[:, 64 * i: 64 * i + 64, :]
            w = chunk.shape[1]
            acc[:, :w, :] = acc[:, :w, :] + chunk
        off = 32
        while off >= 1:
            acc[:, :off, :] = acc[:, :off, :] + acc[:, off: 2 * off, :]
            off //= 2
    return acc[:, 0, :]


def project(results, dirs, basis):
    """results: (P * N,) RADIANCE_DTYPE, probe-major; dirs: the (N, 3) f32 table -> (P,) PROBE_RECORD_DTYPE."""
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    n = len(dirs)
    res = np.ascontiguousarray(results, brt.RADIANCE_DTYPE).reshape(-1, n)
    p = len(res)
    out = np.zeros(p, brt.PROBE_RECORD_DTYPE)
    with np.errstate(all="ignore"):
        rgb = res["rgb"].astype(F32)
        L = (rgb * rgb).astype(F32)                                         # (P, N, 3)
        if basis == SH9:
            Y = sh9_basis(dirs)                                             # (N, 9)
            terms = (Y[None, :, :, None] * L[:, :, None, :]).astype(F32).reshape(p, n, 27)
            sums = _wave_sum(terms)
            scale = F32(12.566371) / F32(n)
            out["coeff"] = (scale * sums).astype(F32)
        else:
            m2 = cube_weights(dirs)                                         # (N, 6)
            num = _wave_sum((m2[None, :, :, None] * L[:, :, None, :]).astype(F32).reshape(p, n, 18)).reshape(p, 6, 3)
            den = _wave_sum(np.broadcast_to(m2[None, :, :], (p, n, 6)).astype(F32))
            val = np.where(den[:, :, None] == 0, F32(0.0), (num / den[:, :, None]).astype(F32))
            out["coeff"][:, :18] = val.reshape(p, 18)
    out["hits"] = ((res["status"] & brt.QUERY_STATUS_HIT) != 0).sum(axis=1)
    out["status"] = res["status"][:, 0] & REFUSED
    out["n_dirs"] = n
    out["basis"] = basis
    refused = out["status"] != 0
    out["coeff"][refused] = 0
    out["hits"][refused] = 0
    return out


def project64(rgb, dirs, basis):
    """The same projection of linear-to-be colours rgb (P, N, 3) in float64, plain sums -> (P, 27)."""
    d = np.asarray(dirs, F32).astype(np.float64).reshape(-1, 3)
    n = len(d)
    L = np.asarray(rgb, F32).astype(np.float64) ** 2
    out = np.zeros((L.shape[0], 27))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    if basis == SH9:
        a, b = float(F32(0.488603)), float(F32(1.092548))
        Y = np.stack([np.full(n, float(F32(0.282095))), a * y, a * z, a * x, b * x * y, b * y * z, float(F32(0.315392)) * (3 * z * z - 1),
                      b * x * z, float(F32(0.546274)) * (x * x - y * y)], axis=1)
        out[:] = (float(F32(12.566371)) / n * np.einsum("nj,pnc->pjc", Y, L)).reshape(-1, 27)
    else:
        c = np.stack([x, -x, y, -y, z, -z], axis=1)
        m2 = np.maximum(c, 0.0) ** 2
        num, den = np.einsum("nf,pnc->pfc", m2, L), m2.sum(axis=0)
        with np.errstate(all="ignore"):
            out[:, :18] = np.where(den[None, :, None] == 0, 0.0, num / den[None, :, None]).reshape(-1, 18)
    return out


def irradiance64(record, normal):
    """brt_host_probe_irradiance in float64 on the record's f32 coefficients -> (3,) float64."""
    c = np.asarray(record["coeff"], F32).astype(np.float64).reshape(27)
    nrm = np.asarray(normal, F32)
    if int(record["basis"]) == SH9:
        Y = sh9_basis(nrm.reshape(1, 3))[0].astype(np.float64)
        return (SH_A[:, None] * c.reshape(9, 3) * Y[:, None]).sum(axis=0)
    n = nrm.astype(np.float64)
    faces = c[:18].reshape(6, 3)
    return sum(n[a] * n[a] * faces[2 * a + (1 if n[a] < 0 else 0)] for a in range(3))


def sky_sh9_analytic():
    """The SH9 coefficients of the linear sky L(d) = (1 - a) + a * top, a = (d_y + 1) / 2 = A + B d_y -> (9, 3) float64."""
    A, B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])
    c = np.zeros((9, 3))
    c[0] = 0.282095 * 4.0 * np.pi * A
    c[1] = 0.488603 * (4.0 * np.pi / 3.0) * B
    return c


def assert_records_equal(got, want, what=""):
    """A NaN exactly where the reference has one; every other word bitwise."""
    assert got.shape == want.shape, what
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 32)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 32)
    gn, wn = np.isnan(got["coeff"]), np.isnan(want["coeff"])
    assert np.array_equal(gn, wn), f"{what}: NaNs differ at {np.argwhere(gn != wn)[:4].tolist()}"
    same = g == w
    same[:, :27] |= wn
    assert same.all(), f"{what}: words differ at {np.argwhere(~same)[:6].tolist()}: got {g[~same][:6]}, want {w[~same][:6]}"
