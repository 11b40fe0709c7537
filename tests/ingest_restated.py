"""NumPy restatements of csrc/ingest.hip, one rounding per operation, with the comparators the GPU tests use and a `mutant=` switch
for the canaries.  TEST INFRASTRUCTURE ONLY; shared by tests/test_cpu_ingest.py and tests/test_gpu_ingest.py.

  undistort_map    k_undistort_map in float64, every product and sum in the order include/gsaj.h writes it -> float32 maps
  ingest_color     k_frame_ingest's colour in float32: the direct path, or the exact bilinear through a map
  ingest_depth     k_frame_ingest's depth: the float64 quotient (or product) rounded to float32 once
  bilinear64       the same bilinear in float64 with a per-pixel bound on what the float32 roundings can add: a check on the mirror
  distort / undistort_points, analytic_image, distorted_source, round_trip   the round trip of the CPU tests

Mutants of the map: "p1_p2_swapped", "k3_dropped", "xd_yd_swapped", "map_x_half".  Of the kernel: "border_clamped" (an outside tap
repeats the edge pixel), "bgr_on_grey" (the BGR swap applied to a one-channel image's planes: plane c reads byte 2 - c of the row),
"round_half_even" (GSAJ_INGEST_ROUND_U8 with rint), "depth_fp32" (the depth divided in float32)."""
import numpy as np

F = np.float32
BGR, ROUND_U8, DEPTH_MUL = 1, 2, 4
MAP_MUTANTS = ("p1_p2_swapped", "k3_dropped", "xd_yd_swapped", "map_x_half")
KERNEL_MUTANTS = ("border_clamped", "bgr_on_grey", "round_half_even", "depth_fp32")

# configs/rgbd/tum/fr1_desk.yaml of the reference at 640 x 480: fx, fy, cx, cy and k1, k2, p1, p2, k3
FR1_K = (517.306408, 516.469215, 318.643040, 255.313989)
FR1_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
SMALL_DIST = (0.12, -0.2, -0.02, 0.015, 0.05)   # tangential terms large enough for their errors to show


def scaled_K(W):
    return tuple(k * (W / 640.0) for k in FR1_K)


def kmat(K):
    fx, fy, cx, cy = K
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def inverse_newK_R(K, R=None, new_K=None):
    """iR of gsaj_undistort_map, formed as gsaj.ingest.UndistortMap forms it."""
    return np.ascontiguousarray(np.linalg.inv(kmat(K if new_K is None else new_K) @ (np.eye(3) if R is None else np.asarray(R, np.float64)))).reshape(-1)


def distort(x, y, dist):
    """Normalised undistorted -> normalised distorted coordinates, float64, in the kernel's order of operations."""
    k1, k2, p1, p2, k3 = (np.float64(d) for d in dist)
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * ((r2 * r2) * r2)
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd, yd


def undistort_map(W, H, K, dist, iR, mutant=None):
    """-> (map_x, map_y) float32 [H,W]."""
    assert mutant is None or mutant in MAP_MUTANTS, mutant
    fx, fy, cx, cy = (np.float64(k) for k in K)
    iR = np.asarray(iR, np.float64).reshape(-1)
    d = list(dist)
    if mutant == "p1_p2_swapped":
        d[2], d[3] = d[3], d[2]
    if mutant == "k3_dropped":
        d[4] = 0.0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = iR[0] * u + iR[1] * v + iR[2]
    Y = iR[3] * u + iR[4] * v + iR[5]
    Wq = iR[6] * u + iR[7] * v + iR[8]
    xd, yd = distort(X / Wq, Y / Wq, d)
    if mutant == "xd_yd_swapped":
        xd, yd = yd, xd
    mx, my = (fx * xd + cx).astype(F), (fy * yd + cy).astype(F)
    if mutant == "map_x_half":
        mx = (mx + F(0.5)).astype(F)
    return mx, my


def _src3(src):
    src = np.asarray(src, np.uint8)
    return src[:, :, None] if src.ndim == 2 else src


def _channel(c, C, flags):
    return 0 if C == 1 else (2 - c if flags & BGR else c)


def _unit(val, flags, mutant=None):
    """A float32 value in grey levels -> [0, 1]."""
    if flags & ROUND_U8:
        val = (np.rint(val) if mutant == "round_half_even" else np.floor((val + F(0.5)).astype(F))).astype(F)
    return np.minimum(np.maximum((val / F(255.0)).astype(F), F(0.0)), F(1.0)).astype(F)


def _taps(src, mx, my, Ws, Hs, clamp):
    """ok [H,W]; ax, ay float32; the four taps' (inside [H,W], yi, xi) with indices made safe."""
    with np.errstate(invalid="ignore"):
        ok = (mx >= F(-1.0)) & (mx <= F(Ws)) & (my >= F(-1.0)) & (my <= F(Hs))   # decided on the floats: NaN and inf fail
    sx, sy = np.where(ok, mx, F(0.0)).astype(F), np.where(ok, my, F(0.0)).astype(F)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - fx0).astype(F), (sy - fy0).astype(F)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
            if clamp:   # the mutant: an outside tap repeats the nearest edge pixel
                inside = np.ones_like(inside)
            taps.append((inside, np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)))
    return ok, ax, ay, taps


def ingest_color(src, flags=0, map_xy=None, mutant=None):
    """src uint8 [Hs,Ws] or [Hs,Ws,C] -> float32 [3,H,W], the kernel's bits."""
    assert mutant is None or mutant in KERNEL_MUTANTS, mutant
    src = _src3(src)
    Hs, Ws, C = src.shape
    assert C in (1, 3, 4)
    if map_xy is None:
        out = np.empty((3, Hs, Ws), F)
        for c in range(3):
            if mutant == "bgr_on_grey" and C == 1 and flags & BGR:   # plane c reads byte 2 - c after the pixel's own
                flat = np.concatenate([src[:, :, 0].reshape(-1), np.zeros(2, np.uint8)])
                plane = flat[np.arange(Hs * Ws) + (2 - c)].reshape(Hs, Ws)
            else:
                plane = src[:, :, _channel(c, C, flags)]
            out[c] = _unit(plane.astype(F), flags & ~ROUND_U8)
        return out
    mx, my = (np.asarray(m, F) for m in map_xy)
    ok, ax, ay, taps = _taps(src, mx, my, Ws, Hs, mutant == "border_clamped")
    bx, by = (F(1.0) - ax).astype(F), (F(1.0) - ay).astype(F)
    out = np.empty((3,) + mx.shape, F)
    for c in range(3):
        ch = _channel(c, C, flags)
        if mutant == "bgr_on_grey" and C == 1 and flags & BGR:
            ch = 0
        p = [np.where(inside, src[yi, xi, ch].astype(F), F(0.0)).astype(F) for (inside, yi, xi) in taps]
        top = ((p[0] * bx).astype(F) + (p[1] * ax).astype(F)).astype(F)
        bot = ((p[2] * bx).astype(F) + (p[3] * ax).astype(F)).astype(F)
        val = ((top * by).astype(F) + (bot * ay).astype(F)).astype(F)
        out[c] = np.where(ok, _unit(val, flags, mutant), F(0.0))
    return out


def ingest_depth(depth_raw, depth_scale, flags=0, mutant=None):
    """uint16 [H,W] -> float32 [H,W]: NumPy's float64 result (depth / scale, or depth * scale) rounded to float32 once."""
    d = np.asarray(depth_raw, np.uint16)
    if mutant == "depth_fp32":
        return (d.astype(F) * F(depth_scale) if flags & DEPTH_MUL else d.astype(F) / F(depth_scale)).astype(F)
    d = d.astype(np.float64)
    return (d * np.float64(depth_scale) if flags & DEPTH_MUL else d / np.float64(depth_scale)).astype(F)


def bilinear64(src, map_xy, flags=0):
    """-> (value float64 [3,H,W] in [0, 1] without GSAJ_INGEST_ROUND_U8's rounding, bound float64 [3,H,W], inside bool [H,W]).
    The float32 mirror may differ from `value` by at most `bound`: the bilinear is three lerps -- 6 products, 3 sums, the two
    complements 1 - a and the fraction a itself, which float32 rounds when the coordinate lies in (-1, 0) -- so 12 roundings of at most
    2^-24 relative each on quantities no larger than the largest tap, then one division whose result, at most 1, is rounded by at most
    2^-25; the clamp adds nothing.  With GSAJ_INGEST_ROUND_U8 the result may differ from `value` by half a grey level more, and by the
    rounding of val + 0.5f, at most 2^-16 of a grey level for val < 256 (2^-15 allowed).
    inside: all four taps lie inside the source."""
    src = _src3(src)
    Hs, Ws, C = src.shape
    mx, my = (np.asarray(m, F) for m in map_xy)
    ok, _, _, taps = _taps(src, mx, my, Ws, Hs, False)
    sx, sy = np.where(ok, mx, 0.0).astype(np.float64), np.where(ok, my, 0.0).astype(np.float64)
    ax, ay = sx - np.floor(sx), sy - np.floor(sy)
    value, bound = np.empty((3,) + mx.shape), np.empty((3,) + mx.shape)
    for c in range(3):
        ch = _channel(c, C, flags)
        p = [np.where(inside, src[yi, xi, ch].astype(np.float64), 0.0) for (inside, yi, xi) in taps]
        val = (p[0] * (1 - ax) + p[1] * ax) * (1 - ay) + (p[2] * (1 - ax) + p[3] * ax) * ay
        value[c] = np.where(ok, np.clip(val / 255.0, 0.0, 1.0), 0.0)
        bound[c] = (12.0 * np.max(p, axis=0) / 255.0 + 0.5) * 2.0 ** -24 + ((0.5 + 2.0 ** -15) / 255.0 if flags & ROUND_U8 else 0.0)
    return value, bound, ok & taps[0][0] & taps[1][0] & taps[2][0] & taps[3][0]


def assert_bits_equal(got, want, tag):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ in their bits, first at %r: got %r want %r" % (tag, int(bad.sum()), bad.size, at, got[at], want[at]))


# ---- the round trip of the CPU tests ------------------------------------------------------------------------------------------------
PHASES = ((0.3, 0.2), (1.1, 0.7), (2.0, 1.3))   # (phi_c, psi_c)


def analytic_image(u, v, W, H):
    """127.5 + 100 sin(a u + phi_c) cos(b v - psi_c), a = 2 pi 1.5 / W, b = 2 pi / H -> float64 [3, ...]; and the largest
    |I_uu| + |I_vv| = 100 (a^2 + b^2)."""
    a, b = 2.0 * np.pi * 1.5 / W, 2.0 * np.pi / H
    img = np.stack([127.5 + 100.0 * np.sin(a * u + phi) * np.cos(b * v - psi) for (phi, psi) in PHASES])
    return img, 100.0 * (a * a + b * b)


def undistort_points(xd, yd, dist, iterations=30):
    """The inverse of distort() by Newton's method in float64 (Jacobian by central differences) -> (x, y, largest residual)."""
    x, y = xd.copy(), yd.copy()
    h = 1e-6
    for _ in range(iterations):
        fx, fy = distort(x, y, dist)
        fxp, fyp = distort(x + h, y, dist)
        fxm, fym = distort(x - h, y, dist)
        gxp, gyp = distort(x, y + h, dist)
        gxm, gym = distort(x, y - h, dist)
        a, c = (fxp - fxm) / (2 * h), (fyp - fym) / (2 * h)
        b, d = (gxp - gxm) / (2 * h), (gyp - gym) / (2 * h)
        det = a * d - b * c
        rx, ry = fx - xd, fy - yd
        x, y = x - (d * rx - b * ry) / det, y - (a * ry - c * rx) / det
    fx, fy = distort(x, y, dist)
    return x, y, float(max(np.abs(fx - xd).max(), np.abs(fy - yd).max()))


def distorted_source(W, H, K, dist):
    """The uint8 [H,W,3] picture a camera with distortion `dist` takes of the analytic image: every source pixel is taken back to
    its undistorted pixel (new_K = K, R = I) and the image evaluated there."""
    fx, fy, cx, cy = K
    vs, us = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y, res = undistort_points((us - cx) / fx, (vs - cy) / fy, dist)
    assert res < 1e-12, res
    img, _ = analytic_image(fx * x + cx, fy * y + cy, W, H)
    return np.ascontiguousarray(np.rint(img).clip(0, 255).astype(np.uint8).transpose(1, 2, 0))


def round_trip(W, H, dist, mutant=None):
    """The distorted source ingested through the (possibly mutated) restated map against the analytic image
    -> (largest |result - truth| in grey levels over the compared pixels, the bound, the compared share of the frame).
    Compared: pixels whose four taps under the CORRECT map are inside the source.  bound = 0.5 + sigma^2 (|I_uu| + |I_vv|)_max / 8:
    0.5 for the source's quantisation, the rest the bilinear's error on an image stretched by at most sigma, the largest
    finite difference of the correct map along u or v."""
    K = scaled_K(W)
    iR = inverse_newK_R(K)
    src = distorted_source(W, H, K, dist)
    good = undistort_map(W, H, K, dist, iR)
    used = good if mutant is None else undistort_map(W, H, K, dist, iR, mutant=mutant)
    got = ingest_color(src, 0, used).astype(np.float64) * 255.0
    _, _, inside = bilinear64(src, good)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    truth, curv = analytic_image(u, v, W, H)
    gx, gy = good[0].astype(np.float64), good[1].astype(np.float64)
    sigma = max(np.hypot(np.diff(gx, axis=1), np.diff(gy, axis=1)).max(), np.hypot(np.diff(gx, axis=0), np.diff(gy, axis=0)).max())
    err = np.abs(got - truth).max(axis=0)
    return float(err[inside].max()), float(0.5 + sigma * sigma * curv / 8.0), float(inside.mean())
