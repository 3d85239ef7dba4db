"""The query matrix of tests/test_gpu_query_lifecycle.py: one row per exported `_dev` query of include/psm_hip.h, a generator of
a small input batch per query family, and a driver that runs every row a handle or a container has and returns the bytes of every
output buffer. Nothing here touches the GPU at import time; tests/test_query_lifecycle_cpu.py holds the table against the header,
so that a query family added later fails there until it has a row here.

A batch is N = 320 queries: five waves, the last lane-partial. The generators are those of the families' own GPU test files
(_random_rays / _nonfinite / _windows, _points / _radii, _sweeps, _around, general_case's poses), imported, not copied; they are
scaled to the triangle set they are given, and each keeps the invalid queries it already makes (NaN, inf, negative radius, empty
window). The list queries run at k = 4 and k = 16, the mesh queries at 4 poses with one reflection among them."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from test_gpu_mesh_query import general_case
from test_gpu_point_query import _points, _radii
from test_gpu_query import _nonfinite, _random_rays, _windows
from test_gpu_world_sweep import _sweeps
from test_gpu_world_tri import _around

F = np.float32
N = 320            # queries per batch: 5 waves, the last one half full
KS = ({"k": 4}, {"k": 16})
ERR_STATE = -5     # PSM_ERR_STATE


def _frame(tris):
    """centre and half diagonal (1 for a set without extent) of a triangle set"""
    p = np.asarray(tris, F).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    return ((lo + hi) * F(0.5)).astype(F), float(np.linalg.norm(hi - lo)) * 0.5 or 1.0


def gen_rays(tris, seed):
    """half from inside the box, half from a shell around it; eight with non-finite or zero parts; a fifth with the plain window
    [0, inf), the rest with _windows' (empty, -inf, +inf, NaN ends), scaled to the scene (no exact-t windows: no hit is known here)"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    rng = np.random.RandomState(seed)
    oi, di = _random_rays(rng, t, N // 2)
    oo, do = _random_rays(rng, t, N - N // 2, outside=True)
    o, d = _nonfinite(np.concatenate([oi, oo]).astype(F), np.concatenate([di, do]).astype(F))
    tmin, tmax = _windows(rng, np.full(N, np.inf, F), N)
    s = F(0.5 * _frame(t)[1])
    tmin, tmax = (tmin * s).astype(F), (tmax * s).astype(F)
    tmin[:N // 5], tmax[:N // 5] = 0, np.inf
    tmin[N // 5:N // 5 + 16] = tmax[N // 5:N // 5 + 16] + F(1)   # empty windows (_windows' own come out as tmin == tmax)
    return {"o": o, "d": d, "tmin": tmin, "tmax": tmax}


def gen_points(tris, seed):
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    rng = np.random.RandomState(seed + 1)
    return {"p": _points(rng, t, N), "r": _radii(rng, N, 0.2 * _frame(t)[1])}


def gen_boxes(tris, seed):
    """boxes over three decades of size around _points' points (its NaN / inf points make invalid boxes); one with lo > hi on an
    axis, one around everything, one point box on a stored vertex"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    rng = np.random.RandomState(seed + 2)
    centre = _points(rng, t, N).astype(np.float64)
    half = _frame(t)[1] * 10.0 ** rng.uniform(-3, -0.3, (N, 1)) * rng.uniform(0.3, 1.0, (N, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0, 0] = hi[0, 0] + F(1)
    pts = t.reshape(-1, 3)
    lo[1], hi[1] = pts.min(0) - F(1), pts.max(0) + F(1)
    lo[2] = hi[2] = t[0, 0]
    return {"lo": lo, "hi": hi}


def gen_sweeps(tris, seed):
    """_sweeps' unit-scale sweeps (the first ten invalid) stretched to the scene"""
    c, h = _frame(tris)
    o, d, r, tm = _sweeps(np.random.RandomState(seed + 3), N, 1.0, 0.3)
    with np.errstate(invalid="ignore"):
        return {"o": (o * F(h) + c).astype(F), "d": (d * F(h)).astype(F), "r": (r * F(h)).astype(F), "tmax": (tm * F(h)).astype(F)}


def gen_tris(tris, seed):
    """_around's triangles over three decades of size around _points' points (the NaN / inf points make invalid triangles); 32 of
    the stored triangles themselves and 8 points on a stored vertex"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    rng = np.random.RandomState(seed + 4)
    centre = _points(rng, t, N).astype(np.float64)
    q = _around(rng, centre, _frame(t)[1] * 10.0 ** rng.uniform(-3, -0.5, (N, 1, 1))).astype(F)
    q[8:40] = t[rng.randint(0, t.shape[0], 32)]
    q[40:48] = t[rng.randint(0, t.shape[0], 8), :1]
    return {"q": q}


def gen_tri_dist(tris, seed):
    q = gen_tris(tris, seed + 5)["q"]
    return {"q": q, "r": _radii(np.random.RandomState(seed + 6), N, 0.2 * _frame(tris)[1])}


@functools.lru_cache(maxsize=None)
def _general_rotations():
    """the rotation parts of general_case()'s poses 0, 1, 2 and 4: the second one a reflection, the others rotations"""
    poses = general_case()[2]
    picked = [np.asarray(poses[k], np.float64) for k in (0, 1, 2, 4)]
    assert [np.linalg.det(m[:, :3]) < 0 for m in picked] == [False, True, False, False]
    return picked


def gen_mesh(tris, seed, into_origin=False):
    """4 poses of the other mesh: general_case()'s rotations (one a reflection) and translations, the latter moved so that a
    unit-sized other mesh stands within half a diagonal of the centre of `tris` -- or, with into_origin, so that the centre of
    `tris`, which then are the OTHER mesh's triangles, comes to lie within half a unit of the origin. r: a radius for the mesh
    clearance queries that some pairs are within and some are not."""
    c, h = _frame(tris)
    rng = np.random.RandomState(seed + 7)
    poses = []
    for m in _general_rotations():
        r, t = m[:, :3], m[:, 3]
        shift = t + rng.uniform(-0.5, 0.5, 3) * (1.0 if into_origin else h)
        poses.append(np.concatenate([r, ((-r @ c if into_origin else c) + shift).reshape(3, 1)], axis=1))
    return {"poses": np.stack(poses), "r": 0.25 * (1.0 if into_origin else h)}


GENERATORS = {"rays": gen_rays, "points": gen_points, "boxes": gen_boxes, "sweeps": gen_sweeps, "tris": gen_tris,
              "tri_dist": gen_tri_dist, "mesh": gen_mesh}
RECORD_BYTES = {"rays": 32, "points": 16, "boxes": 32, "sweeps": 32, "tris": 48, "tri_dist": 48}   # psm_query_ray, psm_point_query, ...

# how a row's Python method takes a batch i and a variant v (k, samples, rmax)
CALLS = {
    "ray": lambda m, i, v: m(i["o"], i["d"], tmin=i["tmin"], tmax=i["tmax"], **v),
    "point": lambda m, i, v: m(i["p"], i["r"]),
    "point_k": lambda m, i, v: m(i["p"], v["k"], i["r"]),
    "inside": lambda m, i, v: m(i["p"], v["samples"]),
    "signed": lambda m, i, v: m(i["p"], i["r"], v["samples"]),
    "box": lambda m, i, v: m(i["lo"], i["hi"], **v),
    "sweep": lambda m, i, v: m(i["o"], i["d"], i["r"], i["tmax"]),
    "tri": lambda m, i, v: m(i["q"], **v),
    "tri_dist": lambda m, i, v: m(i["q"], i["r"]),
    "mesh": lambda m, i, v: m(i["other"], i["poses"], **v),
    "mesh_dist": lambda m, i, v: m(i["other"], i["poses"], i["r"] if v["rmax"] is None else v["rmax"]),
}

# the output buffers of a result by kind: attribute names (None: the result is the array), for a single hierarchy and, with the
# geometry / instance index, for a container; and the bytes per query (per pose "p", per pose and triangle "pt") of every output
# pointer of the C call at k = RAW_K, in the C order
RAW_N, RAW_P, RAW_K, RAW_SAMPLES, RAW_FILL = 64, 2, 4, 3, 0xA5
KINDS = {
    "hits": (("buffer",), ("buffer", "geom"), (16,), (16, 4)),
    "bool": ((None,), (None,), (1,), (1,)),
    "count": ((None,), (None,), (4,), (4,)),
    "lists": (("buffer", "count"), ("buffer", "count", "geom"), (16 * RAW_K, 4), (16 * RAW_K, 4 * RAW_K, 4)),
    "ids": (("tri", "count"), ("tri", "count", "geom"), (4 * RAW_K, 4), (4 * RAW_K, 4 * RAW_K, 4)),
    "tri_hits": (("buffer",), ("buffer", "geom"), (32,), (32, 4)),
    "mesh_bool": ((None,), (None,), (("p", 1),), (("p", 1),)),
    "mesh_count": ((None,), (None,), (("pt", 4),), (("pt", 4),)),
    "mesh_ids": (("tri", "count"), ("tri", "count", "geom"), (("pt", 4 * RAW_K), ("pt", 4)), (("pt", 4 * RAW_K), ("pt", 4 * RAW_K), ("pt", 4))),
    "mesh_hits": (("buffer",), ("buffer", "geom"), (("pt", 32),), (("pt", 32), ("pt", 4))),
    "mesh_pair": (("buffer",), ("buffer", "geom"), (("p", 32),), (("p", 32), ("p", 4))),
}

# a query family: the entry point's name after psm_<owner>_, the method of TriangleHierarchy, of InstanceWorld, and of QueryScene /
# InstancedScene (None: the flat lists have no such query), its generator, its call shape, its variants, its result kind and the
# C call's argument between the batch and the outputs (None, "samples", "k", "rmax")
Family = namedtuple("Family", "name bvh world scene gen call variants kind extra")
ONE = ({},)
SAMPLES = ({"samples": 3},)
FAMILIES = [
    Family("intersect", "intersect", "intersect", "intersect", "rays", "ray", ONE, "hits", None),
    Family("occluded", "occluded", "occluded", "occluded", "rays", "ray", ONE, "bool", None),
    Family("count_hits", "countHits", "countHits", "countHits", "rays", "ray", ONE, "count", None),
    Family("closest_point", "closestPoint", "closestPoint", "closestPoint", "points", "point", ONE, "hits", None),
    Family("within", "within", "within", "within", "points", "point", ONE, "bool", None),
    Family("inside", "inside", "inside", "inside", "points", "inside", SAMPLES, "bool", "samples"),
    Family("signed_distance", "signedDistance", "signedDistance", "signedDistance", "points", "signed", SAMPLES, "hits", "samples"),
    Family("first_hits", "firstHits", "firstHits", None, "rays", "ray", KS, "lists", "k"),
    Family("nearest", "nearest", "nearest", None, "points", "point_k", KS, "lists", "k"),
    Family("box_overlaps", "boxOverlaps", "overlapsBox", None, "boxes", "box", ONE, "bool", None),
    Family("box_count", "boxCount", "countInBox", None, "boxes", "box", ONE, "count", None),
    Family("box_triangles", "boxTriangles", "trianglesInBox", None, "boxes", "box", KS, "ids", "k"),
    Family("sweep_sphere", "sweepSphere", "sphereCast", None, "sweeps", "sweep", ONE, "hits", None),
    Family("sweep_occluded", "sweepOccluded", "sphereCastOccluded", None, "sweeps", "sweep", ONE, "bool", None),
    Family("tri_overlaps", "triOverlaps", "overlapsTriangle", None, "tris", "tri", ONE, "bool", None),
    Family("tri_count", "triCount", "countOnTriangle", None, "tris", "tri", ONE, "count", None),
    Family("tri_triangles", "triTriangles", "trianglesOnTriangle", None, "tris", "tri", KS, "ids", "k"),
    Family("tri_closest", "triClosest", "closestToTriangle", None, "tri_dist", "tri_dist", ONE, "tri_hits", None),
    Family("tri_within", "triWithin", "withinOfTriangle", None, "tri_dist", "tri_dist", ONE, "bool", None),
    Family("mesh_overlaps", "meshOverlaps", "overlapsMesh", None, "mesh", "mesh", ONE, "mesh_bool", None),
    Family("mesh_count", "meshCount", "countOnMesh", None, "mesh", "mesh", ONE, "mesh_count", None),
    Family("mesh_triangles", "meshTriangles", "trianglesOnMesh", None, "mesh", "mesh", KS, "mesh_ids", "k"),
    Family("mesh_closest", "meshClosest", "closestToMesh", None, "mesh", "mesh_dist", ({"rmax": np.inf}, {"rmax": None}), "mesh_hits", "rmax"),
    Family("mesh_within", "meshWithin", "withinOfMesh", None, "mesh", "mesh_dist", ({"rmax": None},), "mesh_bool", "rmax"),
    Family("mesh_clearance", "meshClearance", "clearanceToMesh", None, "mesh", "mesh_dist", ({"rmax": np.inf}, {"rmax": None}), "mesh_pair", "rmax"),
]

# a row of the matrix. export: the C entry point; owner: the Python class that reaches it through `method`; gen, call, variants:
# its family's; outs: the output buffers to compare (attributes of the result; None: the result itself); extra, raw_outs: the C
# call's extra argument and the size of every output pointer (raw_call)
Row = namedtuple("Row", "export owner method gen call variants outs extra raw_outs")


def _rows():
    rows = []
    for f in FAMILIES:
        single, listed, raw_single, raw_listed = KINDS[f.kind]
        rows.append(Row("psm_bvh_%s_dev" % f.name, "TriangleHierarchy", f.bvh, f.gen, f.call, f.variants, single, f.extra, raw_single))
        if f.scene is not None:
            rows.append(Row("psm_scene_%s_dev" % f.name, "QueryScene", f.scene, f.gen, f.call, f.variants, listed, f.extra, raw_listed))
            rows.append(Row("psm_instances_%s_dev" % f.name, "InstancedScene", f.scene, f.gen, f.call, f.variants, listed, f.extra, raw_listed))
        rows.append(Row("psm_world_%s_dev" % f.name, "InstanceWorld", f.world, f.gen, f.call, f.variants, listed, f.extra, raw_listed))
    return rows


ENTRY_POINTS = _rows()


def rows_of(owner):
    name = owner if isinstance(owner, str) else type(owner).__name__
    return [r for r in ENTRY_POINTS if r.owner == name]


def call(obj, row, batch, variant):
    """a row's Python method on obj over a batch (with `other` in it for the mesh queries) at one of its variants"""
    return CALLS[row.call](getattr(obj, row.method), batch, variant)


def run(obj, tris, seed, other=None, only=None, into_origin=False):
    """Every row `obj` (a TriangleHierarchy, QueryScene, InstancedScene or InstanceWorld) has, over batches generated from `tris`
    (the triangles the queries are scaled to: a hierarchy's own, a container's posed ones) and `seed`: {name: result}, the name the
    entry point's with its variant. other: the mesh queries' other hierarchy (None: they are left out); only: the generators to
    keep; into_origin: gen_mesh's."""
    out, batches = {}, {}
    for row in rows_of(obj):
        if (only is not None and row.gen not in only) or (row.gen == "mesh" and other is None):
            continue
        if row.gen not in batches:
            batches[row.gen] = gen_mesh(tris, seed, into_origin) if row.gen == "mesh" else GENERATORS[row.gen](tris, seed)
        batch = dict(batches[row.gen], other=other)
        for v in row.variants:
            tag = "".join(" %s=%s" % (k, "r" if x is None else x) for k, x in sorted(v.items()))
            out[row.export + tag] = (row, call(obj, row, batch, v))
    return out


def buffers(row, result):
    """the output buffers of a row's result as contiguous numpy arrays"""
    return [np.ascontiguousarray(result if a is None else getattr(result, a)) for a in row.outs]


def bytes_of(results):
    """run()'s results reduced to {name: the bytes of every output buffer}"""
    return {name: b"".join(a.tobytes() for a in buffers(row, res)) for name, (row, res) in results.items()}


def answers(obj, tris, seed, other=None, only=None, into_origin=False):
    """every applicable row run over `obj`: {name: the bytes of every output buffer}"""
    return bytes_of(run(obj, tris, seed, other, only, into_origin))


def differing(a, b):
    """the names whose bytes differ between two answers() (or that only one of them has)"""
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def is_miss(row, result):
    """whether a result is its family's miss record on every query: flags false, counts 0, records (u, v, t, tri) = (0, 0, +inf,
    -1) with zeros behind them (a mesh pair's other triangle -1), list slots tri = -1, geometry / instance indices -1"""
    for name, a in zip(row.outs, buffers(row, result)):
        if name == "geom" or name == "tri":
            ok = (a == -1).all()
        elif name == "buffer":
            rec = a.reshape(-1, a.shape[-1])
            ints = rec.view(np.int32)
            ok = not rec[:, :2].any() and np.isposinf(rec[:, 2]).all() and (ints[:, 3] == -1).all()
            if rec.shape[1] == 8:
                pair = getattr(result, "other", None) is not None
                ok = ok and not rec[:, 4:6].any() and not rec[:, 7].any() and ((ints[:, 6] == -1).all() if pair else not rec[:, 6].any())
        else:   # a flag or a count per query, a list's counts
            ok = not a.any()
        if not ok:
            return False
    return True


def raw_call(psm, ctx, row, first, other=None, world=False):
    """The C entry point of a row, called with buffers of its own: RAW_N valid records of zeros (the mesh queries: RAW_P identity
    poses of `other`), every output buffer prefilled with RAW_FILL. first: the leading C arguments (the handle; a list and its
    length). Returns (the return code, the context's message, whether every output buffer still holds the fill)."""
    lib = psm.lib()
    held, outs = [], []

    def buf(nbytes, fill):
        h = ctx.buf_alloc(nbytes)
        held.append(h)
        ctx.buf_upload(h, np.full(nbytes, fill, np.uint8))
        return h, C.c_void_p(ctx.buf_ptr(h)[0])

    extra = {None: (), "samples": (C.c_uint32(RAW_SAMPLES),), "k": (C.c_uint32(RAW_K),), "rmax": (C.c_float(1.0),)}[row.extra]
    try:
        if row.gen == "mesh":
            cells = {"p": RAW_P, "pt": RAW_P * max(int(other.triangleCount), 1)}
            poses = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(12), (RAW_P, 1)))
            args = list(first) + [other._h, poses.ctypes.data_as(C.c_void_p), C.c_size_t(RAW_P)] + ([C.c_int32(-1)] if world else [])
            sizes = [cells[per] * nbytes for per, nbytes in row.raw_outs]
        else:
            args = list(first) + [buf(RECORD_BYTES[row.gen] * RAW_N, 0)[1], C.c_size_t(RAW_N)]
            sizes = [RAW_N * nbytes for nbytes in row.raw_outs]
        for nbytes in sizes:
            h, p = buf(nbytes, RAW_FILL)
            outs.append((h, nbytes))
            args.append(p)
        args[len(args) - len(sizes):len(args) - len(sizes)] = extra
        rc = getattr(lib, row.export)(*args)
        msg = lib.psm_last_error(ctx._h)
        ctx.sync()
        untouched = all((ctx.buf_download(h, np.uint8, nbytes) == RAW_FILL).all() for h, nbytes in outs)
        return rc, msg.decode() if msg else "", untouched
    finally:
        for h in held:
            ctx.buf_free(h)
