"""Poses and worlds at the edges of what an instance world admits, shared by tests/test_world_pose_edges_cpu.py
and tests/test_gpu_world_pose_edges.py: seeded generators in numpy alone, nothing of the device.

The padding and the slacks of the two-level prune rest on three terms: the float32 rounding of the move, 4 eps sqrt 3 (|x| + |T|);
the non-rigidity the pose check admits, R^T R = 1 + E with |E_ij| <= 1e-5; and S, the largest of the object box's |coordinate|,
|T| and the world box's |coordinate|. The case worlds make each of them large:

    far          |T| of 1e2 and 1e4 body sizes (a third of the bodies each, a third near the origin), rotations and reflections
    object_far   meshes stored about 300 units from their object origin and posed back to within a few units of the world origin:
                 S is set by the object box (and by the |T| that undoes it) while the world box is small
    mixed        bodies of size 1e-3, 1 and 1e2 in one world, the small ones beside and inside the boxes of the large
    edge         every pose from edge_pose(): 0.8e-5 < max |E_ij| <= 1e-5
    edge_far     both at once: edge poses at the far shifts, and every fourth body (every second of the cluster at the origin)
                 stored far from its object origin at an edge pose whose rotation is a signed axis permutation -- the forward
                 box is then tight around the body, and the body the candidate tests see stands up to 2.8e-3 outside it

Each world has 48 instances over at most 4 meshes (the 20-triangle icosphere and the 64-triangle torus of the world tests), and
every fifth instance sits exactly at its predecessor's pose: ties. The queries are local to the bodies, half of them as
grid_case() of tests/test_world_query_cpu.py makes them and half aimed at a body's outermost vertex along a world axis; from a
first flat pass a second, decisive one is made per family: tmax at a ray's closest t and one float below it, rmax at a point's
closest distance, boxes that touch posed triangles to within -8 .. 8 ulps, tmax at a sweep's contact, rmax at a triangle's
clearance. At these values a prune that is a hair too tight changes the answer."""
import functools

import numpy as np

import inside_query_model as IQ
import instance_query_model as NQ
import world_box_query_model as WB
import world_query_model as WQ
import world_sweep_query_model as WS
import world_tri_dist_query_model as WD

F = np.float32
D = np.float64
CASES = ("far", "object_far", "mixed", "edge", "edge_far")
INSTANCES = 48
E_LIMIT = 1e-5                     # pose_fault (query.hip): |R^T R - 1| <= 1e-5 on every entry
E_WINDOW = (0.8e-5, 1e-5)          # edge_pose(): the window tests/test_world_box_cpu.py's _edge_pose uses
STORED_AT = (300.0, -200.0, 150.0)  # where the object_far meshes stand in their object space
DRIFT_STEPS = 4096


# ---- poses ------------------------------------------------------------------------------------------------------------------------

def pose_error(pose):
    """max |R^T R - 1| over the nine entries, float64"""
    r = np.asarray(pose, F).reshape(3, 4)[:, :3].astype(D)
    return float(np.abs(r.T @ r - np.eye(3)).max())


def pose_accepted(pose):
    """pose_fault (query.hip) restated in float64: twelve finite numbers, and every dot product of two columns of the float32
    matrix within 1e-5 of 1 or 0"""
    m = np.asarray(pose, F).reshape(3, 4)
    return bool(np.isfinite(m).all()) and not pose_error(m) > E_LIMIT


def rotation(rng, reflect=False):
    """a random rotation (a reflection when `reflect`), float64"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    if reflect:
        q[:, 0] = -q[:, 0]
    return q


def _with_shift(r, t):
    return np.concatenate([np.asarray(r, D), np.asarray(t, D).reshape(3, 1)], axis=1).astype(F)


def edge_pose(rng, reflect, t, base=None):
    """a pose at the edge of the pose check: a double rotation (`base`, or a random one), mirrored when `reflect`, times 1 + s with
    s symmetric, rounded to float32 once; drawn again until 0.8e-5 < max |R^T R - 1| <= 1e-5 in float64. R^T R - 1 = 2 s + s^2:
    half the draws are a pure axis stretch (s and E diagonal), half a shear (s and E off the diagonal)."""
    while True:
        q = rotation(rng) if base is None else np.asarray(base, D)
        if reflect:
            q = q @ np.diag([-1.0, 1.0, 1.0])
        if rng.randint(2) == 0:
            s = np.diag(rng.choice([-1.0, 1.0], 3) * rng.uniform(0.3, 1.0, 3))
        else:
            s = rng.uniform(-1, 1, (3, 3))
            s = (s + s.T) / 2
            s[np.arange(3), np.arange(3)] = 0.0
        s *= 0.4625e-5 / np.abs(s).max()
        p = _with_shift(q @ (np.eye(3) + s), t)
        if E_WINDOW[0] < pose_error(p) <= E_WINDOW[1]:
            return p


def edge_kind(pose):
    """"stretch" or "shear": where the largest entry of R^T R - 1 lies"""
    r = np.asarray(pose, F).reshape(3, 4)[:, :3].astype(D)
    e = np.abs(r.T @ r - np.eye(3))
    return "stretch" if np.diag(e).max() >= e.max() else "shear"


def _mul32(a, b):
    """[n, 3, 3] x [n, 3, 3] in float32, one rounding per product and per sum"""
    return ((a[:, :, 0, None] * b[:, None, 0, :] + a[:, :, 1, None] * b[:, None, 1, :]).astype(F) + a[:, :, 2, None] * b[:, None, 2, :]).astype(F)


def drifted_rotations(rng, steps, count):
    """`count` rotations [count, 3, 3] float32, each composed in float32 from `steps` small rotations (angles up to 0.05 about
    random axes, each rounded to float32): an integrator that never re-orthonormalises. The drift of R^T R grows as a random
    walk, about 1e-7 sqrt(steps)"""
    r = np.repeat(np.eye(3, dtype=F)[None], count, axis=0)
    for _ in range(steps):
        a = rng.normal(size=(count, 3))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        th = rng.uniform(0.01, 0.05, (count, 1, 1))
        k = np.zeros((count, 3, 3))
        k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
        small = np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)
        r = _mul32(r, small.astype(F))
    return r


def drifted_pose(rng, steps=DRIFT_STEPS, t=(0.0, 0.0, 0.0)):
    """a pose whose rotation was composed in float32 from `steps` small rotations -- what pose_fault's bound leaves room for.
    4096 steps is about as far as float32 composition goes under the bound: E between 1e-6 and 1.3e-5, 4.7e-6 in the middle
    (at 16 384 steps half the draws are refused). Drawn again until the pose is accepted with E > 1e-6."""
    while True:
        p = _with_shift(drifted_rotations(rng, steps, 1)[0], t)
        if pose_accepted(p) and pose_error(p) > 1e-6:
            return p


def signed_permutation(rng):
    """a random signed axis permutation that is a rotation, float64: entries 0 and +-1"""
    while True:
        r = np.zeros((3, 3))
        r[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        if np.linalg.det(r) > 0:
            return r


# ---- boxes that touch a posed triangle (from tests/test_world_box_cpu.py, which imports it back) ------------------------------------

def touching_boxes(rng, inst, scale, per):
    """`per` world boxes per triangle of an instance that touch the posed triangle (float64) or miss it by a few ulps: a
    corner, an edge or a face of the box through a vertex, a point of an edge or an interior point, moved by -8 .. 8 ulps"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    v0, e1, e2 = (x.astype(D) for x in WB.posed_leaves(np.asarray(tris, F)[np.sort(cand)], pose))
    t = np.repeat(np.stack([v0, v0 + e1, v0 + e2], axis=1), per, axis=0)
    n = t.shape[0]
    w = rng.uniform(0, 1, (n, 3))
    kind = rng.randint(0, 3, n)
    w[kind == 0] = np.eye(3)[rng.randint(0, 3, (kind == 0).sum())]
    w[kind == 1, rng.randint(0, 3, (kind == 1).sum())] = 0
    w /= w.sum(axis=1, keepdims=True)
    q = (t * w[:, :, None]).sum(axis=1)
    away = -np.sign(t.mean(axis=1) - q)
    away[away == 0] = 1
    ext = 10.0 ** rng.uniform(-3, 0.5, (n, 3)) * scale
    back = np.where(rng.uniform(size=(n, 3)) < 0.3, rng.uniform(0, 1, (n, 3)) * ext, 0)
    nudge = rng.randint(-8, 9, (n, 1)) * np.spacing(np.abs(q).astype(F)).astype(D)
    a, b = q + away * (nudge - back), q + away * (nudge + ext)
    return np.minimum(a, b).astype(F), np.maximum(a, b).astype(F)


# ---- the case worlds ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def base_meshes():
    """the icosphere and the torus of tests/test_gpu_world_query.py's _meshes(): 20 and 64 triangles"""
    return IQ.icosphere(0, 0.6), IQ.torus(8, 4, 0.7, 0.25)


class Case:
    """a case world: meshes [T, 3, 3] float32, entries (mesh index, pose [3, 4] float32), and per instance the radius of its
    body and the world position of its middle (float64), the cluster it stands in, and what the docstrings promise of it"""

    def __init__(self, name, meshes, entries, radius, middle, cluster):
        self.name, self.meshes, self.entries = name, meshes, entries
        self.radius, self.middle, self.cluster = np.asarray(radius, D), np.asarray(middle, D), np.asarray(cluster)
        assert len(entries) == INSTANCES and len(meshes) <= 4 and all(pose_accepted(m) for _, m in entries)

    def insts(self):
        """(tris, cand, pose) of world_query_model: every triangle of these meshes is a leaf"""
        return [(self.meshes[k], np.arange(self.meshes[k].shape[0], dtype=np.int32), m) for k, m in self.entries]

    def box_insts(self):
        """(tris, cand, pose, M) of world_box_query_model, M the plain fit"""
        fit = [WB.plain_fit(t) for t in self.meshes]
        return [(t, c, m, fit[k]) for (t, c, m), (k, _) in zip(self.insts(), self.entries)]

    def members(self):
        """(tris, leaves, M [4, 4], pose) of ray_prune_model: the plain fit extended to 4 x 4"""
        return [(t, c, np.concatenate([M, [[0, 0, 0, 1]]]).astype(F), m) for t, c, m, M in self.box_insts()]


def _place(rng, mesh_middle, r, where):
    """T such that the mesh's middle lands at `where`: where - R middle (float64)"""
    return np.asarray(where, D) - np.asarray(r, D) @ np.asarray(mesh_middle, D)


FAR_ANCHORS = np.array([[0.0, 0.0, 0.0], [1e2, -0.6e2, 0.3e2], [-0.7e4, 1e4, 0.4e4]])


def _cluster_spots(rng, anchor, count, pitch=1.6, jitter=0.45):
    """`count` spots around an anchor on a grid of `pitch` with a jitter: neighbours touch and overlap now and then"""
    side = int(np.ceil(count ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(side ** 3)[:count]]
    return anchor + (g - (side - 1) / 2.0) * pitch + rng.uniform(-jitter, jitter, (count, 3))


def _finish(name, meshes, middles, radii, picks, rot_of, spots, cluster):
    """entries from per-instance picks (mesh index), rotations and spots; every fifth instance at its predecessor's pose"""
    entries, radius, middle = [], [], []
    for k in range(INSTANCES):
        if k % 5 == 4:
            entries.append((entries[-1][0], entries[-1][1].copy()))
            radius.append(radius[-1])
            middle.append(middle[-1])
            cluster[k] = cluster[k - 1]
            continue
        j = picks[k]
        pose = rot_of(k, j, spots[k])
        entries.append((j, pose))
        radius.append(radii[j])
        middle.append(NQ.to_world(pose, np.asarray(middles[j], D)[None])[0])
    return Case(name, meshes, entries, radius, middle, cluster)


@functools.lru_cache(maxsize=None)
def case(name):
    ico, tor = base_meshes()
    rng = np.random.RandomState(7000 + CASES.index(name))
    stored = np.asarray(STORED_AT)
    if name in ("far", "edge", "edge_far"):
        anchors = FAR_ANCHORS if name != "edge" else FAR_ANCHORS[:1]
        cluster = np.arange(INSTANCES) % len(anchors)
        spots = np.zeros((INSTANCES, 3))
        for a in range(len(anchors)):
            at = np.nonzero(cluster == a)[0]
            spots[at] = _cluster_spots(rng, anchors[a], at.size)
        if name == "far":
            meshes, middles, radii = [ico, tor], [np.zeros(3)] * 2, [0.6, 0.95]
            picks = [k % 2 for k in range(INSTANCES)]

            def rot_of(k, j, where):
                return _with_shift(rotation(rng, bool(k & 2)), where)
        else:
            on_axis = np.array([0.0, 0.0, 300.0])
            meshes = [ico, tor, (ico + F(stored)).astype(F), (ico + F(on_axis)).astype(F)]
            middles, radii = [np.zeros(3), np.zeros(3), stored, on_axis], [0.6, 0.95, 0.6, 0.6]
            # edge_far: every fourth body, and every second of the cluster at the origin, is stored far from its object origin
            picks = [(2 + (k // 2) % 2 if name == "edge_far" and (k % 4 == 1 or k % 6 == 3) else k % 2) for k in range(INSTANCES)]

            def rot_of(k, j, where):
                base = signed_permutation(rng) if j >= 2 else None
                p = edge_pose(rng, bool(k & 2), np.zeros(3), base)
                p[:, 3] = _place(rng, middles[j], p[:, :3].astype(D), where).astype(F)
                return p
        return _finish(name, meshes, middles, radii, picks, rot_of, spots, cluster)
    if name == "object_far":
        on_axis = np.array([0.0, 0.0, 300.0])
        meshes = [(ico + F(stored)).astype(F), (tor + F(stored)).astype(F), (ico + F(on_axis)).astype(F), tor]
        middles, radii = [stored, stored, on_axis, np.zeros(3)], [0.6, 0.95, 0.6, 0.95]
        picks = [k % 4 for k in range(INSTANCES)]
        spots = _cluster_spots(rng, np.zeros(3), INSTANCES)

        def rot_of(k, j, where):
            r = rotation(rng, bool(k & 2)) if k % 3 else signed_permutation(rng)
            return _with_shift(r, _place(rng, middles[j], _with_shift(r, np.zeros(3))[:, :3].astype(D), where))
        return _finish(name, meshes, middles, radii, picks, rot_of, spots, np.zeros(INSTANCES, int))
    assert name == "mixed"
    meshes = [(ico * F(1e-3)).astype(F), ico, tor, (ico * F(1e2)).astype(F)]
    middles, radii = [np.zeros(3)] * 4, [0.6e-3, 0.6, 0.95, 0.6e2]
    picks = [3 if k % 12 == 2 else (0 if k % 3 != 1 else 1 + (k // 3) % 2) for k in range(INSTANCES)]
    spots = np.zeros((INSTANCES, 3))
    big = [k for k in range(INSTANCES) if picks[k] == 3]
    unit = [k for k in range(INSTANCES) if picks[k] in (1, 2)]
    for k in big:
        spots[k] = rng.uniform(-70, 70, 3)

    def beside(where, r):
        u = rng.normal(size=3)
        return where + u / np.linalg.norm(u) * r
    for k in unit:                                   # at the surface of a large body: inside its box
        spots[k] = beside(spots[big[rng.randint(len(big))]], 60.0 * rng.uniform(0.85, 1.1))
    for k in range(INSTANCES):
        if picks[k] == 0:                            # beside a unit body, or at the surface of a large one
            spots[k] = beside(spots[unit[rng.randint(len(unit))]], rng.uniform(0.5, 0.9)) if rng.randint(3) else \
                beside(spots[big[rng.randint(len(big))]], 60.0 * rng.uniform(0.99, 1.01))

    def rot_of(k, j, where):
        return _with_shift(rotation(rng, bool(k & 2)), where)
    return _finish(name, meshes, middles, radii, picks, rot_of, spots, np.asarray(picks).copy())


# ---- queries ------------------------------------------------------------------------------------------------------------------------

def seen_vertices(c, i):
    """the vertices of instance i where the candidate tests see them, float64 [V, 3]: T + R^-T v, the world points whose exact move
    is v -- not the forward image R v + T that the world box bounds; the two differ by the pose's non-rigidity"""
    k, pose = c.entries[i]
    m = pose.astype(D)
    v = np.unique(c.meshes[k].reshape(-1, 3), axis=0).astype(D)
    return np.linalg.solve(m[:, :3].T, v.T).T + m[:, 3]


def local_queries(c, seed, n):
    """n rays (o, d, tmin, tmax) and n points (p, rmax) local to bodies of case c, in units of each body's radius, and the body
    each was made for. Half are spread as grid_case()'s: origins within three radii of a random body's middle, aimed at points
    within one radius of it, windows of 1.5 .. 12 radii; points within two radii, rmax of 0.3 .. 3 radii. The other half is aimed
    at the outermost vertex of a body along a world axis (where the candidate tests see it: seen_vertices()), from 0.3 .. 1.5
    radii outside along that axis: with tmax at the hit, or rmax at the distance, the query touches the body at the one place
    where nothing but the padding stands between the world box and it. Bodies stored far from their object origin get all six
    axis directions, the others one."""
    rng = np.random.RandomState(seed)
    half = n // 2
    at = rng.randint(0, INSTANCES, n - half)
    mid, rad = c.middle[at], c.radius[at][:, None]
    o = (mid + rng.uniform(-1, 1, (n - half, 3)) * 3 * rad).astype(F)
    d = (mid + rng.uniform(-1, 1, (n - half, 3)) * rad - o.astype(D)).astype(F)
    p = (mid + rng.uniform(-1, 1, (n - half, 3)) * 2 * rad).astype(F)
    stored_far = [np.abs(c.meshes[k]).max() > 100 for k, _ in c.entries]
    aims = [(i, a, s) for i in range(INSTANCES) for a in range(3) for s in (-1.0, 1.0) if stored_far[i]]
    aims += [(i, rng.randint(3), rng.choice([-1.0, 1.0])) for i in range(INSTANCES) if not stored_far[i]]
    aims = [aims[j] for j in rng.permutation(len(aims))[:half]]
    while len(aims) < half:
        aims.append((rng.randint(INSTANCES), rng.randint(3), rng.choice([-1.0, 1.0])))
    to, td, tp = [], [], []
    for i, a, s in aims:
        x = seen_vertices(c, i)
        v = x[np.argmax(s * x[:, a])]
        out = np.zeros(3)
        out[a] = s
        start = (v + c.radius[i] * rng.uniform(0.3, 1.5) * (out + 0.3 * rng.uniform(-1, 1, 3) * (1 - np.abs(out)))).astype(F)
        to.append(start)
        td.append((v - start.astype(D)).astype(F))
        tp.append((v + c.radius[i] * (rng.uniform(0.1, 1.0) * out + 1e-3 * rng.uniform(-1, 1, 3))).astype(F))
    at = np.concatenate([at, [i for i, _, _ in aims]])
    o, d, p = np.concatenate([o, to]), np.concatenate([d, td]), np.concatenate([p, tp])
    tmin, tmax = np.zeros(n, F), (rng.uniform(1.5, 12.0, n) * c.radius[at]).astype(F)
    rmax = (rng.uniform(0.3, 3.0, n) * c.radius[at]).astype(F)
    return (o, d, tmin, tmax), (p, rmax), at


def decisive_rays(insts, rays):
    """the rays twice: tmax exactly at the flat closest t, and one float below it (a ray without a hit keeps its tmax)"""
    o, d, tmin, tmax = rays
    t = WQ.flat_rays(WQ.per_instance_rays(insts, o, d, tmin, tmax))[0][:, 2]
    hit = np.isfinite(t)
    at, below = np.where(hit, t, tmax).astype(F), np.where(hit, np.nextafter(t, F(-np.inf)), tmax).astype(F)
    return np.concatenate([o, o]), np.concatenate([d, d]), np.concatenate([tmin, tmin]), np.concatenate([at, below])


def decisive_points(insts, points):
    """rmax exactly at the flat closest distance"""
    p, _ = points
    dist = WQ.flat_points(WQ.per_instance_points(insts, p, np.full(p.shape[0], np.inf, F)))[0][:, 2]
    return p, dist.astype(F).copy()


def local_boxes(c, seed, n):
    """n boxes over three decades of size (in body radii) around points near random bodies"""
    rng = np.random.RandomState(seed)
    at = rng.randint(0, INSTANCES, n)
    mid, rad = c.middle[at], c.radius[at][:, None]
    centre = mid + rng.uniform(-1, 1, (n, 3)) * rad
    half = 10.0 ** rng.uniform(-3, 0, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3)) * rad
    return (centre - half).astype(F), (centre + half).astype(F)


def decisive_boxes(c, seed, per_instance=10):
    """boxes that touch posed triangles at a vertex, an edge or a face, moved by -8 .. 8 ulps: per_instance triangles of every
    instance, one box each"""
    rng = np.random.RandomState(seed)
    lo, hi = [], []
    for (tris, cand, pose), rad in zip(c.insts(), c.radius):
        a, b = touching_boxes(rng, (tris, rng.permutation(cand)[:per_instance], pose), rad, 1)
        lo.append(a)
        hi.append(b)
    return np.concatenate(lo), np.concatenate(hi)


def local_sweeps(c, seed, n):
    """n sweeps (o, d, r, tmax = +inf): the local rays' lines, radii over 1e-3 .. 0.5 body radii"""
    (o, d, _, _), _, at = local_queries(c, seed, n)
    rng = np.random.RandomState(seed + 1)
    r = (10.0 ** rng.uniform(-3, np.log10(0.5), n) * c.radius[at]).astype(F)
    return o, d, r, np.full(n, np.inf, F)


def decisive_sweeps(insts, sweeps):
    """tmax at the contact's t (a sweep without a contact keeps +inf)"""
    o, d, r, tm = sweeps
    t = WS.flat(insts, o, d, r, tm)[0][:, 2]
    return o, d, r, np.where(np.isfinite(t), t, tm).astype(F)


def local_triangles(c, seed, n):
    """n world triangles of 0.03 .. 0.8 body radii around points near random bodies, and their rmax: a third +inf, the rest
    0.03 .. 3 radii"""
    rng = np.random.RandomState(seed)
    at = rng.randint(0, INSTANCES, n)
    mid, rad = c.middle[at], c.radius[at][:, None]
    centre = mid + rng.uniform(-1, 1, (n, 3)) * 1.3 * rad
    q = (centre[:, None, :] + rng.normal(size=(n, 3, 3)) * (10.0 ** rng.uniform(-1.5, -0.1, (n, 1, 1)) * rad[:, :, None])).astype(F)
    rm = (10.0 ** rng.uniform(-1.5, 0.5, n) * rad[:, 0]).astype(F)
    rm[::3] = np.inf
    return q, rm


def decisive_triangles(c, seed, q):
    """for the triangle queries: every second triangle gets a forward-posed vertex of a leaf (float32, as the kernels pose it) as
    its first vertex -- it touches there, whatever the rounding of the rest"""
    rng = np.random.RandomState(seed)
    q = q.copy()
    insts = c.insts()
    for i in range(0, q.shape[0], 2):
        tris, cand, pose = insts[rng.randint(INSTANCES)]
        v0 = WB.posed_leaves(tris[rng.randint(len(cand))][None], pose)[0][0]
        q[i] = (q[i] - q[i, :1] + v0).astype(F)
        q[i, 0] = v0
    return q


def decisive_clearance(insts, q):
    """rmax at the flat dist"""
    return WD.flat_near(insts, q, np.inf)[0][:, 2].astype(F).copy()


def other_poses(c, seed, count=6):
    """poses for the other mesh of the mesh queries (the torus): from edge_pose, at bodies of every cluster -- the far shifts
    included --: every second one within a radius of the body's middle, the others about two radii from it"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        pick = np.nonzero(c.cluster == np.unique(c.cluster)[k % len(np.unique(c.cluster))])[0]
        i = pick[rng.randint(pick.size)]
        u = rng.normal(size=3)
        reach = rng.uniform(0.0, 0.8) if k % 2 == 0 else rng.uniform(1.8, 2.4)       # through the body, or beside it
        out.append(edge_pose(rng, bool(k & 1), c.middle[i] + u / np.linalg.norm(u) * reach * max(c.radius[i], 0.5)))
    return out


def far_grid(c, dims=(10, 6, 9)):
    """a grid of `dims` voxels (partial bricks) over the bodies of the case's last cluster -- the far one, where there is one:
    its origin and so its voxel planes are then large float32 numbers --, grown by a body radius. (origin, cell, dims)"""
    pick = np.nonzero(c.cluster == np.unique(c.cluster)[-1])[0]
    if c.name == "mixed":
        pick = pick[:1]
    grow = c.radius[pick].max() * 1.2
    lo, hi = (c.middle[pick] - grow).min(0), (c.middle[pick] + grow).max(0)
    return tuple(float(x) for x in lo), tuple(float(x) for x in (hi - lo) / np.asarray(dims, D)), tuple(dims)
