"""Adaptive rounds on the wavefront pipeline (PT_OPT_ADAPTIVE_WF) without a GPU:
the binding's constant and the option's range, and tests/adaptive_wf_plan_check.cpp
-- plan_adaptive's table under the option, plan_wavefront_adaptive's grids, chunks
and refusals, and the path numbering the two kernels share -- built plainly and
once more under the address and undefined-behaviour sanitizers, each run as a
program of its own."""
import os
import re
import subprocess

import native
import ptamd

SOURCE = os.path.join(native.TESTS, "adaptive_wf_plan_check.cpp")


def test_binding_constant():
    assert ptamd.PT_OPT_ADAPTIVE_WF == 31
    with open(os.path.join(native.INCLUDE, "pathtracer.h")) as f:
        assert re.search(r"^#define PT_OPT_ADAPTIVE_WF 31$", f.read(), re.M)
    taken = [v for k, v in vars(ptamd).items() if k.startswith("PT_OPT_") and k != "PT_OPT_ADAPTIVE_WF"]
    assert 31 not in taken


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-4000:]
    lines = res.stdout.splitlines()
    assert lines[-1].startswith("ok: ") and int(lines[-1].split()[1]) >= 120, lines[-1]
    return lines


def test_plan_table():
    exe = native.build("adaptive_wf_plan_check", [SOURCE], ["-O1"] + native.COMMON[:2] + ["-I", native.CSRC])
    lines = _run(exe)
    assert sum(1 for ln in lines if " wf=1 " in ln) >= 28 and sum(1 for ln in lines if " wf=0 " in ln) >= 42
    assert sum(1 for ln in lines if "refuse_code=-" in ln) >= 27
    assert sum(1 for ln in lines if "chunk=" in ln) >= 20


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = native.build("adaptive_wf_plan_check", [SOURCE],
                       ["-O1", "-g"] + native.COMMON[:2] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                            "-fno-omit-frame-pointer", "-I", native.CSRC],
                       out_dir=tmp_path)
    _run(exe)
