"""The query matrix of tests/query_lifecycle.py against the header (no GPU): every exported `_dev` query of include/psm_hip.h has
a row and every row names an exported query, so a query family added later fails here until it enters the matrix that
tests/test_gpu_query_lifecycle.py walks over a hierarchy's life; every row's Python method exists on its class."""
import inspect
import os
import re

import numpy as np

import query_lifecycle as QL
from util import ROOT


def _header_queries():
    text = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    return re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)


def test_every_exported_query_has_a_row_and_every_row_an_export():
    names = _header_queries()
    assert len(names) == len(set(names)) == 64
    rows = [r.export for r in QL.ENTRY_POINTS]
    assert len(rows) == len(set(rows))
    assert set(names) - set(rows) == set(), "queries of psm_hip.h without a row in query_lifecycle.ENTRY_POINTS"
    assert set(rows) - set(names) == set(), "rows of query_lifecycle.ENTRY_POINTS that psm_hip.h does not export"
    per_owner = {o: len(QL.rows_of(o)) for o in ("TriangleHierarchy", "QueryScene", "InstancedScene", "InstanceWorld")}
    assert per_owner == {"TriangleHierarchy": 25, "QueryScene": 7, "InstancedScene": 7, "InstanceWorld": 25}


def test_every_row_is_complete_and_its_method_exists(psm):
    """(the package imports without a device: no context is made)"""
    assert set(psm.EXPORTS) >= {r.export for r in QL.ENTRY_POINTS}
    prefix = {"TriangleHierarchy": "psm_bvh_", "QueryScene": "psm_scene_", "InstancedScene": "psm_instances_", "InstanceWorld": "psm_world_"}
    for row in QL.ENTRY_POINTS:
        cls = getattr(psm, row.owner)
        assert callable(getattr(cls, row.method, None)), (row.export, row.owner, row.method)
        assert row.export.startswith(prefix[row.owner])
        assert row.gen in QL.GENERATORS and row.call in QL.CALLS and len(row.variants) >= 1 and len(row.outs) >= 1
        assert len(row.raw_outs) == len(row.outs) and row.extra in (None, "samples", "k", "rmax")
        if row.extra == "k":
            assert [v["k"] for v in row.variants] == [4, 16]
        assert (row.gen == "mesh") == ("_mesh_" in row.export)


def test_every_row_calls_its_method_with_arguments_it_takes(psm, scenes):
    """the call shapes bind to the methods' signatures (nothing is run), at every variant"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    batches = {g: f(tris, 3) for g, f in QL.GENERATORS.items()}
    for row in QL.ENTRY_POINTS:
        sig = inspect.signature(getattr(getattr(psm, row.owner), row.method))
        for v in row.variants:
            bound = QL.CALLS[row.call](lambda *a, **k: sig.bind(None, *a, **k), dict(batches[row.gen], other="other"), v)
            for name, value in v.items():
                if value is not None:
                    assert bound.arguments[{"rmax": "r" if "r" in sig.parameters else "rmax"}.get(name, name)] == value, (row.export, name)


def test_is_miss_knows_every_family_s_miss_record(psm):
    """a hand-made miss of every result kind is one; one changed word in any of its buffers is not"""
    hit = np.zeros((5, 4), np.float32)
    hit[:, 2], hit.view(np.int32)[:, 3] = np.inf, -1
    tri_hit = np.zeros((5, 8), np.float32)
    tri_hit[:, 2], tri_hit.view(np.int32)[:, 3] = np.inf, -1
    pair = tri_hit.copy()
    pair.view(np.int32)[:, 6] = -1
    minus, zero = np.full(5, -1, np.int32), np.zeros(5, np.uint32)
    made = {"hits": lambda: psm.QueryHits(hit.copy(), minus.copy()), "bool": lambda: np.zeros(5, np.bool_), "count": lambda: zero.copy(),
            "lists": lambda: psm.QueryHitLists(np.repeat(hit[:, None], 4, axis=1).copy(), zero.copy(), np.full((5, 4), -1, np.int32)),
            "ids": lambda: psm.QueryTriLists(np.full((5, 4), -1, np.int32), zero.copy(), np.full((5, 4), -1, np.int32)),
            "tri_hits": lambda: psm.QueryTriHits(tri_hit.copy(), minus.copy()), "mesh_bool": lambda: np.zeros(5, np.bool_),
            "mesh_count": lambda: np.zeros((5, 3), np.uint32),
            "mesh_ids": lambda: psm.QueryTriLists(np.full((5, 3, 4), -1, np.int32), np.zeros((5, 3), np.uint32), np.full((5, 3, 4), -1, np.int32)),
            "mesh_hits": lambda: psm.QueryTriHits(tri_hit.copy(), minus.copy()), "mesh_pair": lambda: psm.QueryMeshHits(pair.copy(), True, minus.copy())}
    kinds = {f.name: f.kind for f in QL.FAMILIES}
    for row in QL.ENTRY_POINTS:
        kind = kinds[re.match(r"psm_[a-z]+_(\w+)_dev", row.export).group(1)]
        assert QL.is_miss(row, made[kind]()), row.export
        for k in range(len(row.outs)):
            res = made[kind]()
            a = res if row.outs[k] is None else getattr(res, row.outs[k])
            a.reshape(-1)[-1] = 1
            assert not QL.is_miss(row, res), (row.export, row.outs[k])


def test_the_generators_make_full_batches_with_their_invalid_queries(scenes):
    """320 queries each (five waves, the last lane-partial), the invalid ones among them, at every scale the life's states have"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], np.float32)
    point = np.repeat(tri[:, :1], 3, axis=1)
    for tris in (scenes.sponza_like(3001)["tris"].reshape(-1, 3, 3), scenes.cornell()["tris"].reshape(-1, 3, 3),
                 np.concatenate([point, tri, point]), np.concatenate([point] * 4)):
        rays, points, boxes = QL.gen_rays(tris, 5), QL.gen_points(tris, 5), QL.gen_boxes(tris, 5)
        sweeps, q, qd, mesh = QL.gen_sweeps(tris, 5), QL.gen_tris(tris, 5), QL.gen_tri_dist(tris, 5), QL.gen_mesh(tris, 5)
        for batch in (rays, points, boxes, sweeps, q, qd):
            for name, a in batch.items():
                assert a.shape[0] == QL.N == 320 and a.dtype == np.float32, name
        assert np.isnan(rays["d"]).any() and np.isnan(rays["tmin"]).any() and (rays["tmin"] > rays["tmax"]).any()
        assert np.isnan(points["p"]).any() and np.isinf(points["p"]).any() and (points["r"] < 0).any() and np.isnan(points["r"]).any()
        assert np.isnan(boxes["lo"]).any() and (boxes["lo"] > boxes["hi"]).any()
        assert np.isnan(sweeps["o"]).any() and (sweeps["r"] < 0).any() and np.isnan(sweeps["tmax"]).any()
        assert np.isnan(q["q"]).any() and np.isinf(q["q"]).any() and (qd["r"] < 0).any()
        assert mesh["poses"].shape == (4, 3, 4) and sum(np.linalg.det(m[:, :3]) < 0 for m in mesh["poses"]) == 1
        for m in mesh["poses"]:
            assert np.abs(m[:, :3].T @ m[:, :3] - np.eye(3)).max() < 1e-12
