"""numpy restatement of the Doppler kernels' colour operator S_f (csrc/rpt_kernels.hip.h doppler_colour; DESIGN.md "Doppler and
beaming"), in float32 operation for operation — the device probe must equal it bit for bit — and in float64 as the reference it
is checked against."""
import numpy as np

SHIFT, BEAMING = 1, 2
F = np.float32
NU_R = F(546.1 / 700.0)
NU_G = F(1.0)
NU_B = F(546.1 / 435.8)
K0 = F(2.0 * (546.1 / 700.0) - 1.0)
K4 = F(2.0 * (546.1 / 435.8) - 1.0)
KNOTS = (K0, NU_R, NU_G, NU_B, K4)


def spectrum32(u, r, g, b):
    """E_c(u) in float32: piecewise linear through (K0, 0), (NU_R, r), (1, g), (NU_B, b), (K4, 0), 0 outside."""
    u, r, g, b = (np.asarray(x, dtype=np.float32) for x in (u, r, g, b))
    z = np.zeros_like(u)
    seg0, seg1, seg2 = u < NU_R, u < NU_G, u < NU_B
    xa = np.where(seg0, K0, np.where(seg1, NU_R, np.where(seg2, NU_G, NU_B))).astype(np.float32)
    xb = np.where(seg0, NU_R, np.where(seg1, NU_G, np.where(seg2, NU_B, K4))).astype(np.float32)
    ya = np.where(seg0, z, np.where(seg1, r, np.where(seg2, g, b))).astype(np.float32)
    yb = np.where(seg0, r, np.where(seg1, g, np.where(seg2, b, z))).astype(np.float32)
    with np.errstate(all="ignore"):
        t = (u - xa) / (xb - xa)
        e = ya * (F(1) - t) + yb * t
    inside = (u > K0) & (u < K4)
    return np.where(inside, e, z).astype(np.float32)


def S32(D, rgb, flags):
    """S_f(D, c) in float32; D (n,), rgb (n, 3), flags scalar or (n,).  Returns (n, 3) float32."""
    D = np.asarray(D, dtype=np.float32)
    rgb = np.asarray(rgb, dtype=np.float32)
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int64), D.shape)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with np.errstate(all="ignore"):
        sh = np.stack([spectrum32(NU_R / D, r, g, b), spectrum32(NU_G / D, r, g, b), spectrum32(NU_B / D, r, g, b)], axis=1)
        d3 = (D * D) * D
        d2 = D * D
        d4 = d2 * d2
        shifted_beamed = sh * d3[:, None]
        beamed = rgb * d4[:, None]
    out = rgb.copy()
    s = (flags & SHIFT) != 0
    bm = (flags & BEAMING) != 0
    out = np.where((s & bm)[:, None], shifted_beamed, out)
    out = np.where((s & ~bm)[:, None], sh, out)
    out = np.where((~s & bm)[:, None], beamed, out)
    out = np.where((D == F(1))[:, None], rgb, out)
    return out.astype(np.float32)


def spectrum64(u, r, g, b):
    """The same spectrum in float64 (knots as the float32 values the kernel uses)."""
    x = [float(k) for k in KNOTS]
    u = np.asarray(u, dtype=np.float64)
    r, g, b = (np.asarray(c, dtype=np.float64) for c in (r, g, b))
    z = np.zeros_like(u)
    ys = [z, r, g, b, z]
    out = z.copy()
    for i in range(4):
        m = (u > x[i]) & (u <= x[i + 1]) if i else (u > x[0]) & (u <= x[1])
        t = (u - x[i]) / (x[i + 1] - x[i])
        out = np.where(m, ys[i] + (ys[i + 1] - ys[i]) * t, out)
    return np.where(u >= x[4], 0.0, out)


def S64(D, rgb, flags):
    D = np.asarray(D, dtype=np.float64)
    rgb = np.asarray(rgb, dtype=np.float64)
    out = rgb.copy()
    if flags & SHIFT:
        r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        out = np.stack([spectrum64(float(NU_R) / D, r, g, b), spectrum64(1.0 / D, r, g, b), spectrum64(float(NU_B) / D, r, g, b)], axis=1)
        if flags & BEAMING:
            out = out * (D ** 3)[:, None]
    elif flags & BEAMING:
        out = out * (D ** 4)[:, None]
    return out


def kat_inputs(n_random, rng):
    """{D, r, g, b} sets for the known-answer test: D exactly 1, D at and next to every knot crossing of every channel, and D
    log-uniform over [1e-3, 1e3]; colours zero, in [0, 1] and above 1 (lights)."""
    Ds = [np.float32(1.0)]
    for nu in (NU_R, NU_G, NU_B):
        for k in KNOTS:
            d = np.float32(nu / k)          # channel `nu` samples the spectrum at knot k (up to rounding)
            Ds += [d, np.nextafter(d, np.float32(0)), np.nextafter(d, np.float32(np.inf))]
            for s in range(2, 6):
                Ds += [np.float32(d + np.float32(s) * (np.nextafter(d, np.float32(np.inf)) - d)),
                       np.float32(d - np.float32(s) * (d - np.nextafter(d, np.float32(0))))]
    Ds = np.array(Ds, dtype=np.float32)
    special = np.repeat(Ds, 16)
    Dr = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=n_random)).astype(np.float32)
    D = np.concatenate([special, Dr])
    n = D.shape[0]
    c = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    big = rng.random(n) < 0.2
    c[big] *= np.float32(40.0)
    c[rng.random(n) < 0.05] = 0.0
    c[rng.random((n, 3)) < 0.05] = 0.0
    return D, c
