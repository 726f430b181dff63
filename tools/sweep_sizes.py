#!/usr/bin/env python3
"""The sweep walk (PT_OPT_SMALL_SWEEP) on against off by scene size: device
time per 512x512 8-spp frame on one context, interleaved launches, for
random_triangles(4..32) and grid_mesh(2..4).  Prints one line per scene:
triangles, distinct boxes, ms off, ms on (mean and min), on/off.
  python tools/sweep_sizes.py [--reps 30] > profiles/<tag>/sweep_sizes.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "discovering-path-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptamd  # noqa: E402
import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    cases = [(f"random_triangles({n})", scenes.random_triangles(n), scenes.camera((0.3, 0.2, 2.2)))
             for n in (4, 8, 16, 32)]
    cases += [(f"grid_mesh({n})", scenes.grid_mesh(n), scenes.camera((0.0, 0.0, 3.0))) for n in (2, 3, 4)]
    cases.append(("box.obj", None, scenes.DEFAULT_CAMERA))
    print(f"# {a.size}x{a.size} {a.spp} spp, depth 4, sss 3, one context, {a.reps} interleaved launches each; device ms")
    print("# scene tris boxes off_mean off_min on_mean on_min on/off(mean) bitwise")
    for name, arrays, cam in cases:
        scene = (ptamd.Scene.load_obj(scenes.BOX_OBJ) if arrays is None else ptamd.Scene.from_arrays(*arrays)).build_bvh()
        rs, imgs, info = [], [], (0, 0)
        for sweep in (0, 1):
            r = ptamd.Renderer(0)
            r.set_option(ptamd.PT_OPT_SMALL_SWEEP, sweep)
            r.upload(scene)
            r.upload_lights(scenes.REFERENCE_LIGHT)
            r.set_camera(cam)
            r.set_params(4, 3)
            r.resize_and_clear(a.size, a.size)
            for _ in range(16):   # warm-up: the mixed-lane schedule measures itself on the first frames and then settles
                r.clear()
                r.render(0, a.spp)
            imgs.append(r.read_accum())
            if sweep:
                info = r.sweep_info()
            r.set_option(ptamd.PT_OPT_LAUNCH_TIMING, 1)
            r.reset_launch_times()
            rs.append(r)
        for _ in range(a.reps):
            for r in rs:
                r.clear()
                r.render(0, a.spp)
                r.synchronize()
        t = [r.launch_times_ms() for r in rs]
        same = np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
        print(f"{name} {info[1]} {info[0]} {t[0].mean():.4f} {t[0].min():.4f} {t[1].mean():.4f} {t[1].min():.4f} "
              f"{t[1].mean() / t[0].mean():.3f} {'same' if same else 'DIFFERENT'}")
        for r in rs:
            r.close()


if __name__ == "__main__":
    main()
