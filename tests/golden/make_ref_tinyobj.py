"""Regenerates tests/golden/ref_tinyobj.json: the array sizes and SHA-256
digests of what the reference's own OBJ loader (oracle/_ref/libref_tinyobj.so,
`make -C oracle ref`) returns for every file of tests/obj_cases.py.
Needs that library, so it runs only where the reference tree exists; the
tests check the recorded digests against the library whenever it is there."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)
import obj_cases as T  # noqa: E402

if T.ref_lib() is None:
    raise SystemExit("the reference loader's library is absent and cannot be built here")
cases = {name: T.case_record(text) for name, text in sorted(T.CASES.items())}
fuzz = {}
for key, text in T.fuzz_files():
    v, i, _, m = T.ref_parse(text)
    fuzz[key] = T.digest(v, i, m)
with open(T.GOLDEN, "w") as f:
    json.dump({"generator": "tests/golden/make_ref_tinyobj.py",
               "digest": "SHA-256 over each array's length (uint64) and its 32-bit little-endian words",
               "cases": cases, "fuzz": fuzz}, f, indent=1)
    f.write("\n")
print(f"{len(cases)} cases, {len(fuzz)} fuzz files -> {T.GOLDEN}")
