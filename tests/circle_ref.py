"""Exact plane geometry for the cluster-shape tests: the convex hull, the minimum enclosing circle and the containment
predicates on fractions.Fraction of the input doubles.  Nothing here rounds: a double is a dyadic rational, so a
cluster is brought to one power-of-two denominator and every predicate is integer arithmetic; results leave as
Fractions.  No GPU, no oracle, no numpy arithmetic."""
import math
import random
from fractions import Fraction

SEARCH_MAX = 40  # hulls up to this many vertices: pair and triple search; longer ones: Welzl


def fractions_of(pts):
    """[(Fraction x, Fraction y)] of an array of finite doubles [n, 2]."""
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in pts]


def _scaled(P):
    """Integer points and the common denominator q: P[i] = (X[i] / q, Y[i] / q)."""
    q = 1
    for x, y in P:
        q = max(q, x.denominator, y.denominator)  # powers of two: the largest is the common one
    return [(int(x * q), int(y * q)) for x, y in P], q


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(P):
    """Strict vertices of the convex hull of Fraction points, counter-clockwise from the lowest of the leftmost;
    duplicates merged, points on an edge left out.  One point and two points are their own hull."""
    I, q = _scaled(P)
    pts = sorted(set(I))
    if len(pts) > 2:
        lo, up = [], []
        for p in pts:
            while len(lo) >= 2 and _cross(lo[-2], lo[-1], p) <= 0:
                lo.pop()
            lo.append(p)
        for p in reversed(pts):
            while len(up) >= 2 and _cross(up[-2], up[-1], p) <= 0:
                up.pop()
            up.append(p)
        pts = lo[:-1] + up[:-1]
    return [(Fraction(x, q), Fraction(y, q)) for x, y in pts]


def on_hull_edge(p, H):
    """True when the Fraction point p lies on the boundary of the hull H (a vertex included)."""
    h = len(H)
    if h == 1:
        return p == H[0]
    for i in range(h):
        a, b = H[i], H[(i + 1) % h]
        if _cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
            return True
    return False


# A circle over integer points is (ux, uy, D, n): centre (ux / D, uy / D), radius^2 = n / D^2, D > 0.
def _c1(a):
    return a[0], a[1], 1, 0


def _c2(a, b):
    return a[0] + b[0], a[1] + b[1], 2, (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def _c3(a, b, c):
    bx, by, cx, cy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
    D = 2 * (bx * cy - by * cx)
    if D == 0:
        return None
    b2, c2 = bx * bx + by * by, cx * cx + cy * cy
    ux, uy = cy * b2 - by * c2, bx * c2 - cx * b2  # centre - a, times D
    if D < 0:
        D, ux, uy = -D, -ux, -uy
    return a[0] * D + ux, a[1] * D + uy, D, ux * ux + uy * uy


def _holds(c, p):
    dx, dy = p[0] * c[2] - c[0], p[1] * c[2] - c[1]
    return dx * dx + dy * dy <= c[3]


def _smaller(a, b):
    return b is None or a[3] * b[2] * b[2] < b[3] * a[2] * a[2]


def _search(I):
    """The smallest circle through 2 or 3 of the points that holds all of them."""
    h = len(I)
    if h == 1:
        return _c1(I[0])
    best = None
    for i in range(h):
        for j in range(i + 1, h):
            c = _c2(I[i], I[j])
            if _smaller(c, best) and all(_holds(c, p) for p in I):
                best = c
    for i in range(h):
        for j in range(i + 1, h):
            for k in range(j + 1, h):
                c = _c3(I[i], I[j], I[k])
                if c is not None and _smaller(c, best) and all(_holds(c, p) for p in I):
                    best = c
    return best


def _welzl(I, seed):
    """Welzl's algorithm, move-to-front free iterative form; exact predicates, so no degenerate case goes wrong."""
    I = list(I)
    random.Random(seed).shuffle(I)
    c = None
    for i, p in enumerate(I):
        if c is None or not _holds(c, p):
            c = _c1(p)
            for j in range(i):
                if not _holds(c, I[j]):
                    c = _c2(p, I[j])
                    for k in range(j):
                        if not _holds(c, I[k]):
                            c = _c3(p, I[j], I[k])
                            assert c is not None
    return c


def _out(c, q):
    return Fraction(c[0], c[2] * q), Fraction(c[1], c[2] * q), Fraction(c[3], c[2] * c[2] * q * q)


def min_circle_search(H):
    """(cx, cy, r^2) as Fractions by the pair and triple search over the hull H."""
    I, q = _scaled(H)
    return _out(_search(I), q)


def min_circle_welzl(H, seed=0):
    I, q = _scaled(H)
    return _out(_welzl(I, seed), q)


def min_circle(H):
    """(cx, cy, r^2) as Fractions of the minimum enclosing circle of the hull H (convex_hull's output)."""
    return min_circle_search(H) if len(H) <= SEARCH_MAX else min_circle_welzl(H)


def max_dist2(P, cx, cy):
    """max over the Fraction points of |p - c|^2, exactly (c may be Fractions or doubles)."""
    cx, cy = Fraction(cx), Fraction(cy)
    return max((x - cx) ** 2 + (y - cy) ** 2 for x, y in P)


def _sqrt(f):
    """Square root of a non-negative Fraction as a float, without overflow or underflow of the conversion."""
    if f == 0:
        return 0.0
    e = (f.numerator.bit_length() - f.denominator.bit_length()) // 2 * 2
    return math.ldexp(math.sqrt(float(f / Fraction(2) ** e)), e // 2)


def beyond(d2, r):
    """sqrt(d2) - r for an exact d2 and a double r >= 0, to float accuracy of the DIFFERENCE."""
    r = Fraction(r)
    s = _sqrt(d2) + float(r)
    return 0.0 if s == 0 else float((d2 - r * r) / Fraction(s))


def dist(ax, ay, bx, by):
    return _sqrt((Fraction(ax) - Fraction(bx)) ** 2 + (Fraction(ay) - Fraction(by)) ** 2)


def outside_rectangle(P, corners):
    """How far the worst Fraction point lies outside the quadrilateral with the corners (doubles [4, 2]: u0v0, u1v0,
    u1v1, u0v1), as the largest signed distance beyond the line of one of its four edges; <= 0 when every point is
    inside.  An edge of length zero (the rectangle of a line is a segment) bounds along the direction of the edge
    before it instead; without an area the distance from the line counts on both sides; four equal corners are a
    point."""
    q = [tuple(Fraction(float(v)) for v in corners[i]) for i in range(4)]
    e = [(q[(i + 1) % 4][0] - q[i][0], q[(i + 1) % 4][1] - q[i][1]) for i in range(4)]
    l2 = [x * x + y * y for x, y in e]
    area2 = sum(q[i][0] * q[(i + 1) % 4][1] - q[(i + 1) % 4][0] * q[i][1] for i in range(4))
    sgn = (area2 > 0) - (area2 < 0)
    worst = None
    for x, y in P:
        for i in range(4):
            rx, ry = x - q[i][0], y - q[i][1]
            if l2[i] > 0:
                num, den = e[i][0] * ry - e[i][1] * rx, l2[i]  # > 0: to the left of the edge
                num = -sgn * num if sgn else abs(num)
            elif l2[i - 1] > 0:
                num, den = e[i - 1][0] * rx + e[i - 1][1] * ry, l2[i - 1]
            else:
                num, den = Fraction(_sqrt(rx * rx + ry * ry)), Fraction(1)
            v = math.copysign(_sqrt(num * num / den), num)
            worst = v if worst is None or v > worst else worst
    return worst
