"""OBJ texts and the reference loader's answers to them, shared by
tests/test_host.py, tests/test_ref_tinyobj.py and the fixture generator
tests/golden/make_ref_tinyobj.py: hand-written cases, two generators of
polygons, oracle/_ref/libref_tinyobj.so where it exists and the digests of
tests/golden/ref_tinyobj.json where it does not."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np

import scenes

OBJ_CASES = {
    "formats": b"v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
               b"f 1/1/1 2/1/1 3/1/1\nf 1//1 3//1 4//1\nf -4 -2 -1\n",
    "quads_both_diagonals": b"v 0 0 0\nv 2 0 0\nv 2 1 0\nv 0 1 0\nv 0 0 1\nv 1 0 1\nv 3 1 1\nv 0 1 1\n"
                            b"f 1 2 3 4\nf 5 6 7 8\n",
    "numbers": b"v 1.5e1 -.25 +3\nv 0.000000012345678 1E-3 -0\nv 123456789.123456789 7 1e+2\n"
               b"v 0.1 0.2 0.3\nf 1 2 3\nf 2 3 4\n",
    "shapes_and_comments": b"# c\no A\nv 0 0 0\nv 1 0 0\nv 0 1 0\ng B\nusemtl x\nv 0 0 1\n  f 1 2 3\nf 2 3 4\n",
    "crlf": b"v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n",
    # n-gons: tinyobj ear clipping (tiny_obj_loader.h:1740-1955)
    "ngon_convex_xy": b"v 0 0 0\nv 2 0 0\nv 3 1 0\nv 1 3 0\nv -1 1 0\nf 1 2 3 4 5\n",
    "ngon_concave_offset": b"v 1 1 0\nv 5 1 0\nv 5 5 0\nv 3 2 0\nv 1 5 0\nv 0.5 3 0\nf 1 2 3 4 5 6\nf 6 5 4 3 2 1\n",
    "ngon_planes": b"v 0 0 0\nv 0 2 0\nv 0 3 1\nv 0 1 3\nv 0 -1 1\nv 1 0 0\nv 3 0 1\nv 2 0 3\nv 0.5 0 2\nv 0 0 1\n"
                   b"f 1 2 3 4 5\nf 6 7 8 9 10 1\n",
    "ngon_collinear_start": b"v 0 0 0\nv 1 0 0\nv 2 0 0\nv 2 2 1\nv 0 2 1\nv -1 1 0.5\nv -0.5 0.2 0.1\nf 1 2 3 4 5 6 7\n",
    "ngon_star": b"v 0 3 0\nv 1 1 0\nv 3 1 0\nv 1.5 -0.5 0\nv 2 -3 0\nv 0 -1.5 0\nv -2 -3 0\nv -1.5 -0.5 0\n"
                 b"v -3 1 0\nv -1 1 0\nf 1 2 3 4 5 6 7 8 9 10\n",
}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_tinyobj.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_tinyobj.json")
_REF = None
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(GOLDEN) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def digest(*arrays):
    """SHA-256 over the arrays' lengths and 32-bit little-endian words
    (floats by their bits, indices as uint32)."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a).reshape(-1)
        w = a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)
        h.update(np.uint64(w.size).tobytes())
        h.update(w.astype("<u4").tobytes())
    return h.hexdigest()


def ref_lib():
    """The reference loader's library, built on demand where the reference
    tree exists; None where it does not (the recorded digests then stand in)."""
    global _REF
    if _REF is None:
        if not os.path.exists(REF_SO):
            if not os.path.exists("/root/reference/external/tiny_obj_loader.h"):
                return None
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
        L = ctypes.CDLL(REF_SO)
        sz = ctypes.c_size_t
        P = ctypes.c_void_p
        L.ref_obj_parse.argtypes = [ctypes.c_char_p, sz, P, ctypes.POINTER(sz), P, ctypes.POINTER(sz),
                                    P, ctypes.POINTER(sz), P, ctypes.POINTER(sz)]
        _REF = L
    return _REF


def ref_parse(text: bytes):
    L = ref_lib()
    n = [ctypes.c_size_t() for _ in range(4)]
    rc = L.ref_obj_parse(text, len(text), None, ctypes.byref(n[0]), None, ctypes.byref(n[1]), None,
                         ctypes.byref(n[2]), None, ctypes.byref(n[3]))
    assert rc == 0
    v = np.zeros(max(n[0].value, 1), np.float32)
    i = np.zeros(max(n[1].value, 1), np.uint32)
    t = np.zeros(max(n[2].value, 1), np.float32)
    m = np.zeros(max(n[3].value, 1), np.uint32)
    L.ref_obj_parse(text, len(text), v.ctypes.data, ctypes.byref(n[0]), i.ctypes.data, ctypes.byref(n[1]),
                    t.ctypes.data, ctypes.byref(n[2]), m.ctypes.data, ctypes.byref(n[3]))
    return v[: n[0].value], i[: n[1].value], t[: n[2].value], m[: n[3].value]


def _fmt(x, style, rng):
    if style == 0:
        return repr(float(x))
    if style == 1:
        return f"{x:.9e}"
    if style == 2:
        return f"{x:+.3E}"
    s = f"{x:.7f}"
    return s.replace("0.", ".", 1) if rng.random() < 0.5 else s


def _random_polygons(seed, n_faces=40):
    """Star-shaped and convex polygons of 3..14 corners in random planes, with
    jitter (non-planar) and varied number spellings."""
    rng = np.random.default_rng(seed)
    lines, nv = [], 0
    for _ in range(n_faces):
        k = int(rng.integers(3, 15))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.3, 2.0, k) if rng.random() < 0.6 else np.ones(k)
        pts = np.stack([np.cos(ang) * rad, np.sin(ang) * rad, rng.normal(0, 0.05, k)], 1)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pts = pts @ q.T + rng.uniform(-5, 5, 3)
        if rng.random() < 0.3:
            pts = pts[::-1]
        style = int(rng.integers(0, 4))
        for p in pts:
            lines.append("v " + " ".join(_fmt(c, style, rng) for c in p))
        corners = [str(nv + j + 1) if rng.random() < 0.7 else str(j - k) for j in range(k)]
        if rng.random() < 0.3:
            corners = [c + "/" + str(1 + j % 3) for j, c in enumerate(corners)]
        lines.append("f " + " ".join(corners))
        nv += k
    lines = ["vt 0.5 0.5", "vt 0 1", "vt 1 0"] + lines
    return ("\n".join(lines) + "\n").encode()


def _combs(seed, n_faces=20):
    """Comb-shaped (deeply concave) polygons in the axis planes, exactly planar
    or jittered by 1e-3, some reversed, some with a repeated corner: the ear
    clipper's reflex, overlap and degenerate-cross branches."""
    rng = np.random.default_rng(seed)
    lines, nv = [], 0
    for _ in range(n_faces):
        k = int(rng.integers(2, 8))
        pts = []
        for j in range(k):
            pts += [(2 * j, 0), (2 * j + 1, rng.uniform(1, 4))]
        pts += [(2 * k, 0), (2 * k, -1), (0, -1)]
        if rng.random() < 0.3:
            pts = pts[::-1]
        ax = rng.permutation(3)
        for a, b in pts:
            p = [0.0, 0.0, 0.0]
            p[ax[0]], p[ax[1]] = a, b
            p[ax[2]] = float(rng.normal(0, 1e-3)) if rng.random() < 0.5 else 0.0
            lines.append("v %r %r %r" % tuple(float(c) for c in p))
        idx = list(range(nv + 1, nv + len(pts) + 1))
        if rng.random() < 0.3:
            idx.insert(2, idx[2])
        lines.append("f " + " ".join(map(str, idx)))
        nv += len(pts)
    return ("\n".join(lines) + "\n").encode()


CASES = dict(OBJ_CASES)
CASES["box.obj"] = open(scenes.BOX_OBJ, "rb").read()
for _s in range(6):
    CASES[f"random_polygons_{_s}"] = _random_polygons(_s)
    CASES[f"combs_{_s}"] = _combs(_s)


def fuzz_files():
    """(key, text) of the 200 generated files of the fuzz test."""
    for seed in range(100, 200):
        yield f"random_polygons_{seed}", _random_polygons(seed)
        yield f"combs_{seed}", _combs(seed)


def case_record(text):
    """What the golden file keeps of a case: the reference loader's array
    sizes and a digest of each array (vertices, indices, uvs, materials)."""
    v, i, t, m = ref_parse(text)
    return {"sizes": [int(v.size), int(i.size), int(t.size), int(m.size)],
            "v": digest(v), "i": digest(i), "t": digest(t), "m": digest(m)}
