"""What the footprint tests share, on the CPU and on the GPU
(PT_OPT_CULL_FOOTPRINT): the extra cases, the pixel mask of a footprint set as
the kernel evaluates it, and the count of samples the footprints let the
kernel skip."""
import numpy as np

import ptamd
import scenes
from cull_support import CASES, culled_mask, rng_draws

# two lights whose footprints overlap on screen, and a light seen edge-on (the camera lies in its plane)
OVERLAP = np.concatenate([scenes.REFERENCE_LIGHT,
                          ptamd.pack_light([0.8, 1.7, 0.4], [0.0, -1.0, 0.3], [3, 2, 1], [1.5, 1.0])])
FOOT_CASES = CASES + [
    ("two_overlap", scenes.DEFAULT_CAMERA, 96, 54, OVERLAP),
    ("edge_on", scenes.camera((0.0, 2.0, 5.0)), 80, 60, scenes.REFERENCE_LIGHT),
]
FOOT_IDS = [c[0] for c in FOOT_CASES]
LO, HI = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)   # box.obj root


def foot_mask(foot, W, H):
    """The pixels inside some footprint, evaluated as the kernel does: float32
    NDC origins, float32 products and sum, no contraction."""
    px = np.arange(W, dtype=np.float32)
    py = np.arange(H, dtype=np.float32)
    nx = (np.float32(2.0) * px / np.float32(W)) - np.float32(1.0)
    ny = (np.float32(2.0) * py / np.float32(H)) - np.float32(1.0)
    X, Y = np.meshgrid(nx, ny)
    inside = np.zeros((H, W), bool)
    for f in np.asarray(foot, np.float32).reshape(-1, 16):
        m = (X >= f[0]) & (X <= f[1]) & (Y >= f[2]) & (Y <= f[3])
        for k in range(4):
            a, b, c = f[4 + 3 * k], f[5 + 3 * k], f[6 + 3 * k]
            m &= (a * X + b * Y) <= c
        inside |= m
    return inside


def sure_masks(cam, W, H, lights, foot=None):
    """Per light the pixels whose skipped samples are (intensity, 1): inside
    the light's sure region and outside the footprint of the root box and of
    every other light (the kernel's pixel_skip).  None without footprints."""
    if foot is None:
        foot = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights)
    sure, n = ptamd.primary_cull_sure(cam, W, H, LO, HI, lights)
    if foot is None or sure is None:
        return None
    assert len(sure) == len(foot) - 1
    out = []
    for l in range(len(sure)):
        others = np.delete(foot, l + 1, axis=0)
        out.append(foot_mask(sure[l], W, H) & foot_mask(foot[l + 1], W, H) & ~foot_mask(others, W, H))
    return out


def blocks(mask, W, H):
    """Which 16x4 pixel blocks (the wave footprint at one lane per pixel) hold a pixel of the mask."""
    by = -(-H // 4)
    pad = np.zeros((by * 4, W), bool)
    pad[:H] = mask
    return pad.reshape(by, 4, W // 16, 16).any((1, 3))


def foot_skip_counts(cam, W, H, lights, first_batch, n_batches):
    """What include/pathtracer.h defines for PT_OPT_CULL_FOOTPRINT, counted on
    the host: (live pixels, samples the kernel must skip, samples of the same
    pixels it must trace) over the batches.  The pixels are the live ones (inside
    a loose rectangle) outside every footprint or in a sure region
    (sure_masks); a sample of theirs is skipped
    when draws 0 and 2 of seed (batch * H + y) * W + x, after fmax(1e-38, .),
    are both at least u0."""
    loose = ptamd.primary_cull_rects(cam, W, H, LO, HI, lights)
    _, u0 = ptamd.primary_cull_rects_r(cam, W, H, LO, HI, lights)
    foot = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights)
    assert loose is not None and foot is not None and len(loose) == len(foot)
    u0 = np.float32(u0)
    live = ~culled_mask(loose, W, H)
    skippable = ~foot_mask(foot, W, H)
    for m in sure_masks(cam, W, H, lights, foot):
        skippable |= m
    ys, xs = np.nonzero(live & skippable)
    skipped = traced = 0
    for batch in range(first_batch, first_batch + n_batches):
        seeds = (np.uint64(batch) * np.uint64(H) + ys.astype(np.uint64)) * np.uint64(W) + xs.astype(np.uint64)
        u = np.maximum(np.float32(1e-38), rng_draws(seeds, 3))
        skip = (u[:, 0] >= u0) & (u[:, 2] >= u0)
        skipped += int(skip.sum())
        traced += int((~skip).sum())
    return int(live.sum()), skipped, traced
