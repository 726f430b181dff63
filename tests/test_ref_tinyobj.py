"""Pins OBJ ingest against the reference's own loader.

oracle/_ref/libref_tinyobj.so is the reference's vendored tinyobjloader
(external/tiny_obj_loader.h, compiled unmodified where it lies by
`make -C oracle ref`, wrapped as the reference's call site
VulkanRayTracer.cpp:64-92 uses it).  Both restatements -- the product's
pt_scene_parse_obj (csrc/scene/obj_loader.cpp) and the oracle's
oracle_obj_parse -- must reproduce its vertex floats bit for bit and its
triangle index order exactly: the order decides the BVH the builder makes
(BoundingVolumeHierarchy.cpp:25-82) and so every traversal tie-break.

Where the reference tree (and so the library) is absent, the same checks run
against tests/golden/ref_tinyobj.json: SHA-256 digests of the arrays the
reference loader returned for every file these tests use, recorded by
tests/golden/make_ref_tinyobj.py.  With the library present the recorded
digests are checked against it as well, so they cannot go stale.
"""
import numpy as np
import pytest

import oracle_lib as O
import ptamd
from obj_cases import CASES, case_record, digest, fuzz_files, golden, ref_lib, ref_parse


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatements_match_reference_tinyobj(case):
    text = CASES[case]
    want = golden()["cases"][case]
    pv, pi, _, pt, pm = ptamd.Scene.parse_obj(text).arrays()
    ov, oi, ot = O.obj_parse(text)
    if ref_lib() is not None:
        rv, ri, rt, rm = ref_parse(text)
        assert case_record(text) == want, "tests/golden/ref_tinyobj.json no longer matches the reference loader"
        for name, v, i in (("product", pv, pi), ("oracle", ov, oi)):
            assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32)), f"{name} vertices"
            assert np.array_equal(i, ri), f"{name} triangle index order"
        assert np.array_equal(pt.view(np.uint32), rt.view(np.uint32)) and np.array_equal(ot.view(np.uint32),
                                                                                        rt.view(np.uint32))
        assert np.array_equal(pm, rm)
    for name, v, i, t in (("product", pv, pi, pt), ("oracle", ov, oi, ot)):
        assert v.ndim == 1 and digest(v) == want["v"], f"{name} vertices"
        assert digest(i) == want["i"], f"{name} triangle index order"
        assert digest(t) == want["t"], f"{name} uvs"
    assert digest(pm) == want["m"]


def test_reference_loader_box_fixture():
    """The reference loader's box.obj: 8 vertices, 12 triangles, 14 uvs."""
    if ref_lib() is not None:
        v, i, t, m = ref_parse(CASES["box.obj"])
        sizes = [int(v.size), int(i.size), int(t.size), int(m.size)]
        assert sizes == golden()["cases"]["box.obj"]["sizes"]
    else:
        sizes = golden()["cases"]["box.obj"]["sizes"]
    assert sizes == [24, 36, 28, 12]


def test_fuzzed_polygons_match_reference_tinyobj():
    """200 more generated files (both generators): product, oracle and the
    reference loader agree on every vertex bit and triangle index."""
    want = golden()["fuzz"]
    have_ref = ref_lib() is not None
    n = 0
    for key, text in fuzz_files():
        pv, pi, _, _, pm = ptamd.Scene.parse_obj(text).arrays()
        ov, oi, _ = O.obj_parse(text)
        if have_ref:
            rv, ri, _, rm = ref_parse(text)
            assert digest(rv, ri, rm) == want[key], f"{key}: the golden file no longer matches the reference loader"
            assert np.array_equal(pv.view(np.uint32), rv.view(np.uint32)) and np.array_equal(pi, ri), key
            assert np.array_equal(ov.view(np.uint32), rv.view(np.uint32)) and np.array_equal(oi, ri), key
            assert np.array_equal(pm, rm), key
        assert digest(pv, pi, pm) == want[key], key
        assert digest(ov, oi) == digest(pv, pi), key
        n += 1
    assert n == 200 and len(want) == 200
