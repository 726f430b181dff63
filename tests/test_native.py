"""tests/native.py: an output is rebuilt when a file the compiler read for it
changed or the command line did, and only then."""
import os
import subprocess

import native

FLAGS = ["-O1"] + native.COMMON


def _program(tmp_path):
    (tmp_path / "answer.h").write_text("#define ANSWER 41\n")
    (tmp_path / "main.cpp").write_text('#include "answer.h"\nint main() { return ANSWER + EXTRA; }\n')
    (tmp_path / "other.h").write_text("#define OTHER 3\n")
    (tmp_path / "other.cpp").write_text('#include "other.h"\nextern "C" int other() { return OTHER; }\n')
    for name in ("answer.h", "main.cpp", "other.h", "other.cpp"):
        _older(tmp_path / name, 100)
    return [str(tmp_path / "main.cpp"), str(tmp_path / "other.cpp")]   # the header of the first source counts too


def _older(path, seconds=10):
    """Moves a file's mtime back, so that a rebuild or a touch shows whatever the clock's grain."""
    t = os.path.getmtime(path) - seconds
    os.utime(path, (t, t))
    return t


def test_rebuilds_when_a_header_or_a_define_changes_and_only_then(tmp_path):
    srcs = _program(tmp_path)
    out = tmp_path / "out"
    exe = native.build("prog", srcs, FLAGS + ["-DEXTRA=1"], out_dir=out)
    assert exe == str(out / "prog") and subprocess.run([exe]).returncode == 42
    assert os.path.exists(exe + ".d") and os.path.exists(exe + ".argv")

    built = _older(exe)
    assert native.build("prog", srcs, FLAGS + ["-DEXTRA=1"], out_dir=out) == exe
    assert os.path.getmtime(exe) == built, "nothing touched: the output stays"

    for header in ("answer.h", "other.h"):          # named by no list of sources: the compiler's account has them
        os.utime(tmp_path / header)
        native.build("prog", srcs, FLAGS + ["-DEXTRA=1"], out_dir=out)
        assert os.path.getmtime(exe) > built, f"{header} touched: rebuilt"
        built = _older(exe)

    native.build("prog", srcs, FLAGS + ["-DEXTRA=2"], out_dir=out)
    assert os.path.getmtime(exe) > built, "another define: rebuilt"
    assert subprocess.run([exe]).returncode == 43


def test_shared_library_and_a_lost_record(tmp_path):
    srcs = _program(tmp_path)[1:]
    so = native.build("libother.so", srcs, FLAGS, shared=True, out_dir=tmp_path)
    import ctypes
    assert ctypes.CDLL(so).other() == 3
    built = _older(so)
    os.remove(so + ".d")
    native.build("libother.so", srcs, FLAGS, shared=True, out_dir=tmp_path)
    assert os.path.getmtime(so) > built, "no dependency file: rebuilt"
