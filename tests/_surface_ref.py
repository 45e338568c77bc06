"""TEST-ONLY numpy restatement of the GPU iso-surface point sampler (gaussian_gan_decoder_amd/csrc/ggd_surface.hip):
marching tetrahedra over the 6 tetrahedra around every cell's 0-7 diagonal, faces numbered cell by cell (cells in
[x][y][z] order), tetrahedron by tetrahedron; point i sits on face i mod F with weights from the same counter-based
generator.  The mesh family and the sampling rule follow main/decoder_utils/target_dataloader.py:96-118."""
import numpy as np

TET = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
CORNER = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)])
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def corner_values(sigma, level, dtype=np.float32):
    """sigma - level at the 8 corners of every cell, [cells, 8]; the difference is taken in `dtype` (the kernel's: float32)."""
    n = sigma.shape[0]
    m = n - 1
    f = np.empty((m, m, m, 8), dtype)
    for c in range(8):
        dx, dy, dz = CORNER[c]
        f[..., c] = sigma[dx:dx + m, dy:dy + m, dz:dz + m].astype(dtype) - dtype(level)
    return f.reshape(-1, 8)


def cell_face_counts(sigma, level):
    f = corner_values(sigma, level)
    cnt = np.zeros(f.shape[0], np.int64)
    for t in range(6):
        inside = (f[:, TET[t]] > 0).sum(1)
        cnt += np.where((inside == 0) | (inside == 4), 0, np.where(inside == 2, 2, 1))
    return cnt


def _edge(fc, a, b):
    t = fc[a] / (fc[a] - fc[b])
    return CORNER[a].astype(np.float32) + np.float32(t) * (CORNER[b] - CORNER[a]).astype(np.float32)


def face_triangle(sigma, level, offsets, face):
    """Vertices (index coordinates, float32 [3,3]) of face number `face`; offsets = inclusive cumsum of the cell counts."""
    n = sigma.shape[0]; m = n - 1
    cell = int(np.searchsorted(offsets, face, side="right"))
    local = int(face - (offsets[cell - 1] if cell else 0))
    cz, cy, cx = cell % m, (cell // m) % m, cell // (m * m)
    fc = np.array([sigma[cx + CORNER[c][0], cy + CORNER[c][1], cz + CORNER[c][2]] for c in range(8)], np.float32) - np.float32(level)
    for t in range(6):
        ins = [c for c in TET[t] if fc[c] > 0]
        outs = [c for c in TET[t] if not fc[c] > 0]
        nt = 0 if len(ins) in (0, 4) else (2 if len(ins) == 2 else 1)
        if local >= nt:
            local -= nt
            continue
        if len(ins) in (1, 3):
            s = ins[0] if len(ins) == 1 else outs[0]
            o = outs if len(ins) == 1 else ins
            v = [_edge(fc, s, o[0]), _edge(fc, s, o[1]), _edge(fc, s, o[2])]
        else:
            p, q, r, s2 = ins[0], ins[1], outs[0], outs[1]
            v = [_edge(fc, p, r)] + ([_edge(fc, p, s2), _edge(fc, q, s2)] if local == 0 else [_edge(fc, q, s2), _edge(fc, q, r)])
        return np.stack(v) + np.array([cx, cy, cz], np.float32)
    raise AssertionError("face index beyond the cell's triangles")


def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
        return z ^ (z >> np.uint64(31))


def _u01(bits):
    return ((bits & np.uint64(0xFFFFFF)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def point_random_numbers(seed, idx):
    """(w0, w1, w2, thickness gaussian) of output points idx (array of ints), as the kernel draws them."""
    i = np.asarray(idx, np.uint64)
    with np.errstate(over="ignore"):
        h0 = _mix64(np.uint64(seed) ^ ((i * np.uint64(0xD1342543DE82EF95)) & M64))
    h1 = _mix64(h0)
    r0, r1, r2 = _u01(h0), _u01(h0 >> np.uint64(24)), _u01(h1)
    rs = (r0 + r1) + r2
    g1, g2 = _u01(h1 >> np.uint64(24)), _u01(_mix64(h1))
    gauss = np.sqrt(np.float32(-2.0) * np.log(g1)) * np.cos(np.float32(6.283185307179586) * g2)
    return r0 / rs, r1 / rs, r2 / rs, gauss.astype(np.float32)


def all_triangles(sigma, level, corner_dtype=np.float32):
    """Every triangle of the marching-tetrahedra surface, vectorised (the SET the kernel samples from, not its face numbering):
    float64 [F, 3, 3] vertices in index coordinates.  len == cell_face_counts(...).sum().  The corner differences sigma - level
    are the kernel's float32 ones unless corner_dtype = np.float64 (same signs, so the same triangles; the vertices move by the
    rounding of the difference)."""
    n = sigma.shape[0]; m = n - 1
    f = corner_values(sigma, level, corner_dtype).astype(np.float64)        # [cells, 8]
    cell = np.arange(f.shape[0])
    origin = np.stack([cell // (m * m), (cell // m) % m, cell % m], 1).astype(np.float64)
    corner = CORNER.astype(np.float64)
    out = []

    def edge(fc, rows, a, b):                                              # a, b: per-row corner ids
        fa, fb = fc[rows, a], fc[rows, b]
        t = (fa / (fa - fb))[:, None]
        return corner[a] + t * (corner[b] - corner[a])
    for t in range(6):
        ids = TET[t]
        inside = f[:, ids] > 0
        k = inside.sum(1)
        for kk in (1, 2, 3):
            rows = np.nonzero(k == kk)[0]
            if rows.size == 0:
                continue
            ins = inside[rows]
            # stable order: the `kk` inside vertices first (kk = 1, 2) / the outside vertex first (kk = 3), each group in TET order
            key = ~ins if kk in (1, 2) else ins
            order = np.argsort(key, axis=1, kind="stable")
            v = ids[order]                                                 # [rows, 4] corner ids
            if kk in (1, 3):
                tri = np.stack([edge(f, rows, v[:, 0], v[:, j]) for j in (1, 2, 3)], 1)
                out.append(tri + origin[rows][:, None, :])
            else:
                p, q, r, s2 = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
                e_pr, e_ps, e_qs, e_qr = edge(f, rows, p, r), edge(f, rows, p, s2), edge(f, rows, q, s2), edge(f, rows, q, r)
                out.append(np.stack([e_pr, e_ps, e_qs], 1) + origin[rows][:, None, :])
                out.append(np.stack([e_pr, e_qs, e_qr], 1) + origin[rows][:, None, :])
    return np.concatenate(out, 0) if out else np.zeros((0, 3, 3))


def triangle_areas(tri):
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


# ------------------------------------------------------------------------------- whole passes, vectorised -----
def _cell_origins(n):
    m = n - 1
    cell = np.arange(m * m * m)
    return np.stack([cell // (m * m), (cell // m) % m, cell % m], 1)


def _numbered_face_corners(sigma, level):
    """(cell [F], ab [F, 3, 2]): for every face in the kernel's numbering (cell by cell in [x][y][z] order, tetrahedron
    0..5, local triangle 0 / 1) its cell and, per vertex, the two LOCAL corner ids (a, b) of the cut edge the vertex lies
    on, a being the corner the interpolation starts from (edge_point(f, a, b) of the kernel)."""
    f = corner_values(sigma, level)
    cells = f.shape[0]
    ab = np.zeros((cells, 6, 2, 3, 2), np.int8)
    valid = np.zeros((cells, 6, 2), bool)
    for t in range(6):
        ids = TET[t]
        inside = f[:, ids] > 0
        k = inside.sum(1)
        # the lone corner first (k = 1: the inside one, k = 3: the outside one) / the two inside corners first (k = 2),
        # each group in TET order
        key = np.where((k == 3)[:, None], inside, ~inside)
        v = ids[np.argsort(key, axis=1, kind="stable")]                      # [cells, 4] corner ids
        lone = (k == 1) | (k == 3)
        s = v[:, 0]
        one = np.stack([np.stack([s, v[:, j]], 1) for j in (1, 2, 3)], 1)    # (s o0)(s o1)(s o2)
        p, q, r, s2 = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
        pr, ps, qs, qr = (np.stack(e, 1) for e in ((p, r), (p, s2), (q, s2), (q, r)))
        two0, two1 = np.stack([pr, ps, qs], 1), np.stack([pr, qs, qr], 1)
        ab[:, t, 0] = np.where(lone[:, None, None], one, two0)
        ab[:, t, 1] = two1
        valid[:, t, 0] = (k >= 1) & (k <= 3)
        valid[:, t, 1] = k == 2
    cell = np.broadcast_to(np.arange(cells)[:, None, None], valid.shape)[valid]
    return cell, ab[valid]


def numbered_faces(sigma, level):
    """Every face in the kernel's numbering with float32 vertex arithmetic: float32 [F, 3, 3], row i bit-equal to
    face_triangle(sigma, level, offsets, i)."""
    n = sigma.shape[0]
    f = corner_values(sigma, level)
    cell, ab = _numbered_face_corners(sigma, level)
    a, b = ab[..., 0], ab[..., 1]
    fa, fb = f[cell[:, None], a], f[cell[:, None], b]
    t = (fa / (fa - fb)).astype(np.float32)
    corner = CORNER.astype(np.float32)
    local = corner[a] + t[..., None] * (CORNER[b] - CORNER[a]).astype(np.float32)
    return (local + _cell_origins(n)[cell].astype(np.float32)[:, None, :]).astype(np.float32)


def face_vertex_ids(sigma, level):
    """[F, 3, 2] global corner pairs (lo, hi) naming each face vertex by the grid edge it lies on, faces in the kernel's
    numbering.  A vertex whose outside corner sits exactly at the level lies ON that corner, whichever edge led there:
    it is named (corner, corner), so that the vertices which collapse onto one corner are one vertex."""
    n = sigma.shape[0]
    f = corner_values(sigma, level)
    cell, ab = _numbered_face_corners(sigma, level)
    g = _cell_origins(n)[cell][:, None, None, :] + CORNER[ab]                # [F, 3, 2, 3] grid coordinates
    gid = (g[..., 0] * n + g[..., 1]) * n + g[..., 2]                        # [F, 3, 2]
    fa, fb = f[cell[:, None], ab[..., 0]], f[cell[:, None], ab[..., 1]]
    on = np.where(fa == 0, gid[..., 0], np.where(fb == 0, gid[..., 1], -1))    # the corner the vertex sits on, if any
    lo, hi = np.minimum(gid[..., 0], gid[..., 1]), np.maximum(gid[..., 0], gid[..., 1])
    return np.stack([np.where(on >= 0, on, lo), np.where(on >= 0, on, hi)], -1)


def edge_uses(sigma, level):
    """How often each undirected edge between two DISTINCT vertices occurs in the triangle set.  Returns (edges [E, 2, 2]:
    the two vertices of each edge as face_vertex_ids names them, uses [E], collapsed: the number of triangles with two
    vertices on one corner -- their area is zero and the edge between the twins is not counted)."""
    n = sigma.shape[0]
    vid = face_vertex_ids(sigma, level)
    key = vid[..., 0] * (n ** 3) + vid[..., 1]                               # [F, 3] one integer per vertex
    collapsed = int(((key[:, 0] == key[:, 1]) | (key[:, 1] == key[:, 2]) | (key[:, 0] == key[:, 2])).sum())
    u = np.concatenate([key[:, 0], key[:, 1], key[:, 2]])
    v = np.concatenate([key[:, 1], key[:, 2], key[:, 0]])
    keep = u != v
    lo, hi = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
    pairs, uses = np.unique(np.stack([lo, hi], 1), axis=0, return_counts=True) if lo.size else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    edges = np.stack([pairs // (n ** 3), pairs % (n ** 3)], -1)              # [E, 2 vertices, 2 corners]
    return edges, uses, collapsed


def kuhn_interpolant(sigma, level, p):
    """The float64 piecewise-linear interpolant of sigma - level on the six tetrahedra around each cell's 0-7 diagonal, at
    index coordinates p [N, 3]; its zero set IS the iso-surface.  No case table: the cell by floor, the fractions sorted in
    descending order, and a walk from corner 0 along those axes."""
    g = np.asarray(sigma, np.float64) - float(level)
    n = g.shape[0]
    p = np.asarray(p, np.float64).reshape(-1, 3)
    cell = np.clip(np.floor(p), 0, n - 2).astype(np.int64)
    frac = p - cell
    order = np.argsort(-frac, axis=1, kind="stable")
    rows = np.arange(p.shape[0])
    cur = cell.copy()
    val = g[cur[:, 0], cur[:, 1], cur[:, 2]].copy()
    for k in range(3):
        ax = order[:, k]
        nxt = cur.copy()
        nxt[rows, ax] += 1
        val += frac[rows, ax] * (g[nxt[:, 0], nxt[:, 1], nxt[:, 2]] - g[cur[:, 0], cur[:, 1], cur[:, 2]])
        cur = nxt
    return val


def cell_scale(sigma, level, p):
    """D of the interpolant bound: the largest |sigma - level| over the corners of the cell that holds p (cell by floor,
    clipped as in kuhn_interpolant)."""
    g = np.abs(np.asarray(sigma, np.float64) - float(level))
    n = g.shape[0]
    cell = np.clip(np.floor(np.asarray(p, np.float64).reshape(-1, 3)), 0, n - 2).astype(np.int64)
    d = np.zeros(cell.shape[0])
    for c in range(8):
        q = cell + CORNER[c]
        d = np.maximum(d, g[q[:, 0], q[:, 1], q[:, 2]])
    return d


def interpolant_ratio(sigma, level, out_points):
    """|kuhn_interpolant| / (2^-24 n D) of OUTPUT points (index / n - 0.5), mapped back to index coordinates in float64.  Where
    D = 0 (a cell with every corner at the level: the interpolant vanishes on all of it) the ratio is 0, or inf if it does not."""
    n = sigma.shape[0]
    idx = (np.asarray(out_points, np.float64) + 0.5) * n
    val = np.abs(kuhn_interpolant(sigma, level, idx))
    scale = 2.0 ** -24 * n * cell_scale(sigma, level, idx)
    return np.where(scale > 0, val / np.where(scale > 0, scale, 1.0), np.where(val > 0, np.inf, 0.0))


def restated_points(sigma, level, seed, num_points, faces=None):
    """The float32 restatement of a whole thickness-0 call: point i = ((w0 v0 + w1 v1) + w2 v2) / n - 0.5 on face i mod F."""
    n = sigma.shape[0]
    faces = numbered_faces(sigma, level) if faces is None else faces
    F = len(faces)
    if F == 0 or num_points == 0:
        return np.zeros((num_points, 3), np.float32)
    i = np.arange(num_points)
    w0, w1, w2, _ = point_random_numbers(seed, i)
    tri = faces[i % F]
    idx = (w0[:, None] * tri[:, 0] + w1[:, None] * tri[:, 1]) + w2[:, None] * tri[:, 2]
    return (idx / np.float32(n) - np.float32(0.5)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ fields -----
FIELD_SEED = 20240611


def _zero_boundary(s):
    s[0], s[-1] = 0, 0
    s[:, 0], s[:, -1] = 0, 0
    s[:, :, 0], s[:, :, -1] = 0, 0
    return s


def make_field(name, n, corner=0):
    """float32 [n, n, n] test fields with a fixed seed (level 10 unless said otherwise):
    noise  uniform(0, 20), the six boundary slabs 0     -- all sign patterns, closed surface
    ties   integers 8..12, same boundary                -- many corners exactly at the level
    steep  0 or 3e4 with probability 1/2, same boundary -- interpolation parameter next to 0 / 1
    open   noise without the zeroed boundary            -- the surface leaves the grid
    one_corner  grid corner `corner` at 20, the rest 0   -- single-cell faces (n = 2: THE cell's corner `corner`)
    empty / full  nothing / everything above the level  -- no faces"""
    rng = np.random.default_rng([FIELD_SEED, n, {"ties": 1, "steep": 2}.get(name, 0)])      # open = noise before its boundary is zeroed
    if name in ("noise", "open"):
        s = rng.uniform(0.0, 20.0, (n, n, n)).astype(np.float32)
        return _zero_boundary(s) if name == "noise" else s
    if name == "ties":
        return _zero_boundary(rng.integers(8, 13, (n, n, n)).astype(np.float32))
    if name == "steep":
        return _zero_boundary(np.where(rng.random((n, n, n)) < 0.5, np.float32(0.0), np.float32(3e4)).astype(np.float32))
    if name == "one_corner":
        s = np.zeros((n, n, n), np.float32)
        s[tuple((n - 1) * CORNER[corner])] = 20.0
        return s
    if name == "empty":
        return np.zeros((n, n, n), np.float32)
    if name == "full":
        return np.full((n, n, n), 20.0, np.float32)
    raise ValueError(name)


# Bound of the GPU tests on |kuhn_interpolant| of an output point: K 2^-24 n D.  K_MEASURED is the largest such ratio of the
# float32 restatement's own points over every field of the GPU tests (test_surface_fields_host.py measures it again), K = 4 x.
K_MEASURED = 7.56
K_INTERPOLANT = 4.0 * K_MEASURED

ROUGH = ("noise", "ties", "steep", "open")
ROUGH_SIZES = (9, 14, 17, 18)


def small_fields():
    """(id, field) of every small field the GPU tests run: the rough ones at n = 9, 14, 17, 18, the single-cell and the
    faceless ones at n = 2 and 3."""
    out = [(f"{name}-{n}", make_field(name, n)) for name in ROUGH for n in ROUGH_SIZES]
    out += [(f"one_corner{c}-{n}", make_field("one_corner", n, c)) for n in (2, 3) for c in range(8)]
    out += [(f"{name}-{n}", make_field(name, n)) for name in ("empty", "full") for n in (2, 3)]
    return out
