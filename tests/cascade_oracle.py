"""numpy restatement of the cascade's rule (scene.py CascadeSceneInference, csrc/scene.hip
unetpp_scene_screen), shared by tests/test_cascade_host.py and tests/test_gpu_cascade.py.

  R_t      = the tile's owned rectangle O_t grown by `margin` on all four sides, clipped to the tile's own extent
  active_t = any(!(v < threshold)) over all classes and all pixels of R_t   (equal activates; a NaN activates)
  score_t  = fmax of the values                                            (a NaN is ignored; -inf when all are NaN)
  out      = where(A, D, M1),  A[s, :, y, x] = active of the tile that owns (y, x)
"""
import numpy as np

from tests.test_scene_host import rect_rows


def screen_rects(H, W, tile, halo, align, margin, frames=1):
    """rows (frame, oy, ox, y_lo, y_hi, x_lo, x_hi) of the screened rectangles of the plan (H, W, tile, halo, align)"""
    th, tw = min(tile, H), min(tile, W)
    out = []
    for (s, oy, ox, y0, y1, x0, x1) in rect_rows(H, W, tile, halo, align, frames):
        out.append((s, oy, ox, max(y0 - margin, oy), min(y1 + margin, oy + th), max(x0 - margin, ox),
                    min(x1 + margin, ox + tw)))
    return out


def screen_ref(maps, rects, threshold):
    """maps float32 [S, C, H, W] (numpy), rows as above -> (active int32 [n], score float32 [n]); frame < 0: (0, -inf)"""
    maps = np.asarray(maps, dtype=np.float32)
    thr = np.float32(threshold)
    active = np.zeros(len(rects), dtype=np.int32)
    score = np.full(len(rects), -np.inf, dtype=np.float32)
    for t, (s, _, _, y0, y1, x0, x1) in enumerate(rects):
        if s < 0:
            continue
        v = maps[s, :, y0:y1, x0:x1].reshape(-1)
        assert v.size > 0
        active[t] = int((~(v < thr)).any())
        score[t] = np.fmax.reduce(v, initial=np.float32(-np.inf))
    return active, score


def owner_mask(rects, active, S, H, W):
    """bool [S, 1, H, W]: the active flag of the tile that owns each pixel (rows carry the OWNED rectangles)"""
    A = np.zeros((S, 1, H, W), dtype=bool)
    for (s, _, _, y0, y1, x0, x1), a in zip(rects, active):
        A[s, :, y0:y1, x0:x1] = bool(a)
    return A
