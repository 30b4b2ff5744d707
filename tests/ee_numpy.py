"""NumPy restatement of the engine's edge-edge contact ("contact_ee", csrc/k_contact.hpp) for tests/test_gpu_contact_ee.py, and the
two-bar scene those tests use: two elastic bars of diamond cross-section (square cells rotated 45 degrees about the bar axis) that cross
ridge over ridge.  Nothing here calls the GPU except bar_context(), which builds an engine context from the tables.

Rules restated (include/tsl_hip.h, tsl_contact_counts):
- edges: the unique edges of each body's surface triangles, ascending (v0, v1), numbered body after body;
- descriptors: query edges = surface edges with both vertices in [v_start, v_end) of every other body the range covers whose pair with
  b_idx no earlier descriptor took; no self pairs; ascending (v0, v1); target edges = the edges of body b_idx, ascending;
- a pair qualifies when the closest points of the two lines lie strictly inside both edges, sin(angle) >= 1e-2 and the line distance is
  below eps_contact; the query edge's vertices are swapped when D = ((b1 - b0) x (a1 - a0)) . (a0 - b0) < 0 (then s -> 1 - s);
- record idx = (b0, b1, a0, a1), w = (s, t, 0); energy 1/2 k (d - eps)^2 (d < eps) + k_f f0(|T (a(s) - b(t) - dx0)|)."""
import numpy as np

SIN_MIN = 1e-2


# ------------------------------------------------------------------------------------------------ bar scene
def _cube_tets(nx, ny, nz):
    """five tets per cube, corner codes XOR-ed with the cube parity (the tet layout of engine/model_elastic_offset.py)"""
    def i2p(I):
        return (I[..., 0] * ny + I[..., 1]) * nz + I[..., 2]
    I = np.stack(np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"), -1).reshape(-1, 3)
    codes = [(j, j ^ 1, j ^ 2, j ^ 4) for j in (0, 3, 5, 6)] + [(1, 2, 4, 7)]
    tets = np.zeros((len(I) * 5, 4), np.int32)
    for slot, vs in enumerate(codes):
        for c, v in enumerate(vs):
            bits = np.array([(v >> k) & 1 for k in range(3)])
            tets[np.arange(len(I)) * 5 + slot, c] = i2p(I + ((bits[None, :] ^ I) & 1))
    G = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    order = np.argsort(i2p(G))
    return tets, G[order]


def _surface(tets, x):
    """faces that belong to one tet only, oriented outwards"""
    faces = {}
    for t in tets:
        for k in range(4):
            f = [t[j] for j in range(4) if j != k]
            key = tuple(sorted(f))
            a, b, c = f
            if np.dot(np.cross(x[b] - x[a], x[c] - x[a]), x[a] - x[t[k]]) < 0:
                b, c = c, b
            faces.setdefault(key, []).append((a, b, c))
    return np.array([v[0] for v in faces.values() if len(v) == 1], np.int32)


def diamond_bar(n, dx, w, angle, center):
    """bar of n nodes along its axis (spacing dx, centred on the axis origin), one w x w cell in cross-section rotated 45 degrees about the
    axis; the axis is x rotated by `angle` about z; returns (x, tets, faces, ridge_top, ridge_bottom) with the ridge vertex ids along the axis"""
    tets, G = _cube_tets(n, 2, 2)
    loc = np.zeros((len(G), 3))
    loc[:, 0] = (G[:, 0] - (n - 1) / 2) * dx
    yz = (G[:, 1:] - 0.5) * w
    c = np.cos(np.pi / 4)
    loc[:, 1] = c * yz[:, 0] - c * yz[:, 1]
    loc[:, 2] = c * yz[:, 0] + c * yz[:, 1]
    ca, sa = np.cos(angle), np.sin(angle)
    R = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    x = loc @ R.T + np.asarray(center, float)
    ridge_top = np.where((G[:, 1] == 1) & (G[:, 2] == 1))[0]
    ridge_bottom = np.where((G[:, 1] == 0) & (G[:, 2] == 0))[0]
    return x, tets, _surface(tets, x), ridge_top, ridge_bottom


def bar_scene(n=6, dx=0.01, w=0.01, gap=5e-4, angle=np.pi / 2, n_up=None, dx_up=None, mu=0.5, density=1000.0, mu_el=2e4, lam_el=3e4):
    """lower bar along x (frozen), upper bar along `angle` above it; the ridges cross at the origin halfway between nodes of both bars
    (n even) with the given gap.  Returns a dict of the tables bar_context() needs plus the ridge ids."""
    n_up = n if n_up is None else n_up
    dx_up = dx if dx_up is None else dx_up
    h = w / np.sqrt(2)
    xl, tl, fl, rl, _ = diamond_bar(n, dx, w, 0.0, (0, 0, 0))
    xu, tu, fu, _, ru = diamond_bar(n_up, dx_up, w, angle, (0, 0, 2 * h + gap))
    nl = len(xl)
    x = np.concatenate([xl, xu])
    tets = np.concatenate([tl, tu + nl])
    faces = np.concatenate([fl, fu + nl])
    NV = len(x)
    elastics, mass = [], np.zeros(NV)
    for off, nv, t in ((0, nl, tl), (nl, len(xu), tu)):
        xx = x[off:off + nv]
        Ds = np.stack([xx[t[:, 0]] - xx[t[:, 3]], xx[t[:, 1]] - xx[t[:, 3]], xx[t[:, 2]] - xx[t[:, 3]]], axis=2)
        W = np.abs(np.linalg.det(Ds)) / 6
        np.add.at(mass, off + t.ravel(), np.repeat(W / 4 * density, 4))
        elastics.append(dict(kind=1, n_verts=nv, n_cells=len(t), v_offset=off, mu=mu_el, lam=lam_el, alpha=0.0, tets=t,
                             B=np.linalg.inv(Ds).reshape(-1, 9), W=W))
    bodies = [(0, nl, 0, len(fl)), (nl, NV, len(fl), len(faces))]
    pairs = [(0, nl, NV, mu), (1, 0, nl, mu)]   # both directions, as BaseScene.contact_pairs lists them
    frozen = np.zeros(3 * NV, np.int32)
    frozen[:3 * nl] = 1
    gravity = np.zeros((NV, 3)); gravity[:, 2] = -9.8
    return dict(x=x, faces=faces, bodies=bodies, pairs=pairs, elastics=elastics, mass=mass, frozen=frozen, gravity=gravity,
                ridge_lower=rl, ridge_upper=ru + nl, n_lower=nl)


def bar_context(sc, k_contact=1000.0, eps_contact=1e-3, dt=5e-3, grid_h=0.003, max_n_constraints=4000):
    from thinshelllab_amd.context import TslContext
    ctx = TslContext(tot_NV=len(sc["x"]), dt=dt, mass=sc["mass"], gravity=sc["gravity"], frozen=sc["frozen"], elastics=sc["elastics"],
                     faces=sc["faces"], bodies=sc["bodies"], pairs=sc["pairs"], k_contact=k_contact, eps_contact=eps_contact,
                     max_n_constraints=max_n_constraints, grid_h=grid_h)
    return ctx


def ridge_distance(x, sc):
    """signed distance of the two ridge lines next to the crossing, positive while the upper ridge is above the lower one"""
    rl, ru = sc["ridge_lower"], sc["ridge_upper"]
    m, k = len(rl) // 2, len(ru) // 2
    p0, p1 = x[rl[m - 1]], x[rl[m]]
    q0, q1 = x[ru[k - 1]], x[ru[k]]
    n = np.cross(p1 - p0, q1 - q0)
    n = n / np.linalg.norm(n)
    if n[2] < 0:
        n = -n
    return float(np.dot(q0 - p0, n))


# ------------------------------------------------------------------------------------------------ detection
def surface_edges(faces, bodies):
    edges, e0 = [], [0]
    for (_, _, f0, f1) in bodies:
        es = set()
        for f in faces[f0:f1]:
            for k in range(3):
                u, v = int(f[k]), int(f[(k + 1) % 3])
                es.add((min(u, v), max(u, v)))
        edges += sorted(es)
        e0.append(len(edges))
    return np.array(edges, np.int64).reshape(-1, 2), e0


def descriptors(pairs, bodies, edges, e0):
    """(pair index, target body, query edge ids) of the descriptors that carry edge-edge contact"""
    out, seen = [], set()
    for pi, p in enumerate(pairs):
        b, v0, v1 = p[0], p[1], p[2]
        q = []
        for bb, bd in enumerate(bodies):   # every other body the range covers, for its first descriptor against b only
            if bb == b or bd[1] <= v0 or bd[0] >= v1 or (min(bb, b), max(bb, b)) in seen:
                continue
            seen.add((min(bb, b), max(bb, b)))
            q += [(edges[e][0], edges[e][1], e) for e in range(e0[bb], e0[bb + 1]) if v0 <= edges[e][0] < v1 and v0 <= edges[e][1] < v1]
        q.sort()
        if q and e0[b + 1] > e0[b]:
            out.append((pi, b, [e for _, _, e in q]))
    return out


def qualifies(a0, a1, b0, b1, eps):
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    aa, ee, ab, c, f = d1 @ d1, d2 @ d2, d1 @ d2, d1 @ r, d2 @ r
    cr = np.cross(d2, d1)
    cc = cr @ cr
    if not (cc >= SIN_MIN * SIN_MIN * aa * ee) or not cc > 0:
        return None
    s = (ab * f - c * ee) / cc
    t = (aa * f - ab * c) / cc
    if not (0 < s < 1 and 0 < t < 1):
        return None
    C = np.sqrt(cc)
    D = cr @ r
    return (s, t, D) if abs(D) / C < eps else None


def record(x, prev, idx, st, k_contact, eps, mu):
    """the remaining fields of an edge-edge slot as k_ee_build writes them: dx0, c_k, n, T (2 x 3)"""
    X, P = x[idx], prev[idx]
    s, t = st
    cr = np.cross(X[1] - X[0], X[3] - X[2])
    C = np.linalg.norm(cr)
    n = cr / C
    gap = (cr @ (X[2] - X[0])) / C
    dx0 = ((1 - s) * P[2] + s * P[3]) - ((1 - t) * P[0] + t * P[1])
    t1 = np.array([n[0], n[2], -n[1]]) if abs(n[0]) < 0.5 else np.array([n[1], -n[0], n[2]])
    t2 = np.cross(n, t1)
    t1 = np.cross(n, t2)
    return dict(dx0=dx0, k=-mu * k_contact * (gap - eps), n=n, T=np.concatenate([t1, t2]))


def brute_force(x, faces, bodies, pairs, eps):
    """the edge-edge list by an O(E^2) search: idx (n, 4), (s, t) (n, 2), in list order"""
    edges, e0 = surface_edges(faces, bodies)
    idx, st = [], []
    for _, b, ql in descriptors(pairs, bodies, edges, e0):
        for eq in ql:
            a0, a1 = edges[eq]
            for et in range(e0[b], e0[b + 1]):
                b0, b1 = edges[et]
                if len({a0, a1, b0, b1}) < 4:
                    continue
                q = qualifies(x[a0], x[a1], x[b0], x[b1], eps)
                if q is None:
                    continue
                s, t, D = q
                if D < 0:
                    idx.append((b0, b1, a1, a0)); st.append((1 - s, t))
                else:
                    idx.append((b0, b1, a0, a1)); st.append((s, t))
    return np.array(idx, np.int64).reshape(-1, 4), np.array(st).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ energy of one constraint (complex-step safe)
def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _f0(x, eh):
    return x if x.real > eh else (-x * x * x / (3 * eh * eh) + x * x / eh + eh / 3)


def line_distance(X):
    """d = (p1 x p2) . p / |p1 x p2|, q = (x1 - x0, x3 - x2, x2 - x0); X: (4, 3)"""
    cr = _cross(X[1] - X[0], X[3] - X[2])
    return (cr @ (X[2] - X[0])) / np.sqrt(cr @ cr)


def energy_normal(X, k_contact, eps):
    d = line_distance(X)
    return 0.5 * k_contact * (d - eps) ** 2 if d.real < eps else 0.0 * d


def energy_friction(X, w, dx0, T, kf, eh):
    s, t = w[0], w[1]
    dx = (1 - s) * X[2] + s * X[3] - (1 - t) * X[0] - t * X[1] - dx0
    T = np.asarray(T).reshape(2, 3)
    u = T @ dx
    return kf * _f0(np.sqrt(u @ u), eh)


def grad_cs(fun, X, h=1e-30):
    """complex-step gradient (12,) of a scalar function of the (4, 3) positions"""
    g = np.zeros(12)
    for i in range(12):
        Z = X.astype(complex)
        Z.flat[i] += 1j * h
        g[i] = fun(Z).imag / h
    return g
