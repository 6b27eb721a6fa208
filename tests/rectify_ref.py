"""Plain restatement of aocr_find_page_quad, aocr_rectify_plan and aocr_warp_page (include/aocr.h).  The quad: the flood fill of
tests/components_ref.py over the paper mask, then integer extremes.  The plan: Python ints, then Python floats (IEEE doubles, one rounding
per operation).  The warp: vectorised float64, one numpy operation per specified operation.  make_photo builds the test photographs.  Test
infrastructure: it does not import the product."""
import math

import numpy as np

import components_ref as CR


def quad_valid(q):
    """q: eight ints x0 y0 .. x3 y3 = TL, TR, BR, BL.  All four cross products (P[i+1]-P[i]) x (P[i+2]-P[i+1]) > 0."""
    p = [(int(q[2 * i]), int(q[2 * i + 1])) for i in range(4)]
    for i in range(4):
        a, b, c = p[i], p[(i + 1) % 4], p[(i + 2) % 4]
        if not (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) > 0:
            return False
    return True


def find_page_quad(page, threshold=-1, dark_paper=0):
    """the 16 int32 words of aocr_find_page_quad."""
    page = np.asarray(page)
    H, W = page.shape
    labels, comps, info = CR.label_components(page, threshold, 0 if dark_paper else 1, 8, max_components=page.size)
    out = np.zeros(16, np.int32)
    out[8], out[10] = info[0], info[2]
    if len(comps) == 0:
        return out
    best = max(comps.tolist(), key=lambda c: (c[5], -c[4]))                    # the largest area, then the smallest label
    ys, xs = np.nonzero(labels == best[4])
    pts = list(zip(xs.tolist(), ys.tolist()))
    tl = min(pts, key=lambda p: (p[0] + p[1], p[1]))
    tr = max(pts, key=lambda p: (p[0] - p[1], -p[1]))
    br = max(pts, key=lambda p: (p[0] + p[1], p[1]))
    bl = min(pts, key=lambda p: (p[0] - p[1], -p[1]))
    q = [*tl, *tr, *br, *bl]
    out[:8] = q
    out[9] = best[5]
    out[11] = 1 if quad_valid(q) else 0
    return out


def rectify_plan(quad, Wo_in=0, Ho_in=0):
    """((Wo, Ho), coef (9) float64); ValueError for a quad that is not valid or an output that is too large."""
    q = [int(v) for v in np.asarray(quad).reshape(-1)]
    if len(q) != 8 or not quad_valid(q):
        raise ValueError("the quad is not convex and clockwise")
    x0, y0, x1, y1, x2, y2, x3, y3 = q
    d2 = lambda ax, ay, bx, by: (ax - bx) ** 2 + (ay - by) ** 2
    Wo = Wo_in if Wo_in > 0 else math.isqrt(max(d2(x1, y1, x0, y0), d2(x2, y2, x3, y3))) + 1
    Ho = Ho_in if Ho_in > 0 else math.isqrt(max(d2(x3, y3, x0, y0), d2(x2, y2, x1, y1))) + 1
    if Wo > 16384 or Ho > 16384 or Wo * Ho > 1 << 26:
        raise ValueError(f"the rectified page would be {Wo} x {Ho}")
    dx1, dx2, dx3 = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, dy3 = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den, gn, hn = dx1 * dy2 - dy1 * dx2, dx3 * dy2 - dy3 * dx2, dx1 * dy3 - dy1 * dx3
    g, h = float(gn) / float(den), float(hn) / float(den)
    a, b, c = float(x1 - x0) + g * float(x1), float(x3 - x0) + h * float(x3), float(x0)
    d, e, f = float(y1 - y0) + g * float(y1), float(y3 - y0) + h * float(y3), float(y0)
    U, V = float(max(Wo - 1, 1)), float(max(Ho - 1, 1))
    UV = U * V
    return (Wo, Ho), np.array([a * V, b * U, c * UV, d * V, e * U, f * UV, g * V, h * U, UV], np.float64)


def warp_points(coef, x, y):
    """(X, Y, dn) float64 for pixel coordinates x, y (arrays)."""
    c = np.asarray(coef, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        nx = c[0] * x
        nx = nx + c[1] * y
        nx = nx + c[2]
        ny = c[3] * x
        ny = ny + c[4] * y
        ny = ny + c[5]
        dn = c[6] * x
        dn = dn + c[7] * y
        dn = dn + c[8]
        return nx / dn, ny / dn, dn


def warp_page(page, coef, fill, Ho, Wo):
    """(Ho, Wo) uint8."""
    page = np.asarray(page)
    H, W = page.shape
    y, x = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    X, Y, dn = warp_points(coef, x, y)
    with np.errstate(all="ignore"):
        ok = (dn > 0) & (X >= -1.0) & (X <= float(W)) & (Y >= -1.0) & (Y <= float(H))
        X, Y = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
        qx = np.floor(X * 256.0 + 0.5).astype(np.int64)
        qy = np.floor(Y * 256.0 + 0.5).astype(np.int64)
    ix, iy, fx, fy = qx >> 8, qy >> 8, qx & 255, qy & 255

    def tap(tx, ty):
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        return np.where(inside, page[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), int(fill))

    top = tap(ix, iy) * (256 - fx) + tap(ix + 1, iy) * fx
    bot = tap(ix, iy + 1) * (256 - fx) + tap(ix + 1, iy + 1) * fx
    out = (top * (256 - fy) + bot * fy + 32768) >> 16
    return np.where(ok, out, int(fill)).astype(np.uint8)


def rectify(photo, quad, fill=255, Wo_in=0, Ho_in=0):
    """the photograph warped through the plan of `quad`: what recognize_page(rectify=quad) reads."""
    (Wo, Ho), coef = rectify_plan(quad, Wo_in, Ho_in)
    return warp_page(photo, coef, fill, Ho, Wo)


def inside_quad(quad, H, W):
    """(H, W) bool: the pixel centre (x, y) is inside or on the integer-cornered polygon (exact integer cross products)."""
    p = [(int(quad[2 * i]), int(quad[2 * i + 1])) for i in range(4)]
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    ok = np.ones((H, W), bool)
    for i in range(4):
        a, b = p[i], p[(i + 1) % 4]
        ok &= (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0]) >= 0
    return ok


def make_photo(page, quad, H, W, desk):
    """an (H, W) uint8 photograph of `page` lying with its corners at `quad` (TL, TR, BR, BL) on a desk of gray `desk`: paper pixels sample
    the page bilinearly through the inverse of the plan's map, desk pixels are `desk`."""
    page = np.asarray(page)
    Hp, Wp = page.shape
    _, coef = rectify_plan(quad, Wp, Hp)
    inv = np.linalg.inv(coef.reshape(3, 3))
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    w = inv[2, 0] * x + inv[2, 1] * y + inv[2, 2]
    u = np.clip((inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]) / w, 0.0, Wp - 1.0)
    v = np.clip((inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]) / w, 0.0, Hp - 1.0)
    iu, iv = np.minimum(u.astype(np.int64), Wp - 2 if Wp > 1 else 0), np.minimum(v.astype(np.int64), Hp - 2 if Hp > 1 else 0)
    fu, fv = u - iu, v - iv
    iu1, iv1 = np.minimum(iu + 1, Wp - 1), np.minimum(iv + 1, Hp - 1)
    p = page.astype(np.float64)
    val = (p[iv, iu] * (1 - fu) + p[iv, iu1] * fu) * (1 - fv) + (p[iv1, iu] * (1 - fu) + p[iv1, iu1] * fu) * fv
    paper = inside_quad(quad, H, W)
    return np.where(paper, np.clip(np.floor(val + 0.5), 0, 255), desk).astype(np.uint8)
