"""The per-point image-feature query of tools/extract_image_feature.py:84-100, restated: a Python loop over the lidar
rows with ``int()``, the maps as a dict camera id -> (C, H, W) array, the result a dict row -> float32 [C].

``query`` is the loop with the library's documented deviation made explicit: where the reference would raise
(IndexError for an index past the map, ValueError / OverflowError from ``int()`` of a NaN or an infinity) or silently
wrap a negative index, the row is left out and counted.  Values that are finite but no int32 are counted too."""
import math

import numpy as np


def _int(v):
    """int(v) as the loop applies it; None where the library refuses the value."""
    v = float(v)
    if not math.isfinite(v) or abs(v) >= 2.0 ** 31:
        return None
    return int(v)


def query(lidar, maps, cp_col=6):
    """-> (features: dict row -> float32 [C], cameras: dict row -> camera id, number of refused rows)."""
    features, cameras, outside = dict(), dict(), 0
    for i in range(lidar.shape[0]):
        point = lidar[i, :]
        chosen = None
        bad = False
        for k in (cp_col, cp_col + 3):
            name = _int(point[k])
            if name is None:
                bad = True
                break
            if (name - 1) in maps:
                chosen = (name - 1, _int(point[k + 1]), _int(point[k + 2]))
                break
        if bad:
            outside += 1
            continue
        if chosen is None:
            continue
        camera_id, image_x, image_y = chosen
        fmap = maps[camera_id]
        if image_x is None or image_y is None or not (0 <= image_x < fmap.shape[2] and 0 <= image_y < fmap.shape[1]):
            outside += 1
            continue
        features[i] = np.asarray(fmap[:, image_y, image_x]).astype(np.float32)
        cameras[i] = camera_id
    return features, cameras, outside


def dense(features, cameras, n, channels):
    """The two dicts as the library's outputs: float32 [n, C] with zero rows, int32 [n] with -1."""
    out = np.zeros((n, channels), dtype=np.float32)
    cam = np.full((n,), -1, dtype=np.int32)
    for i, v in features.items():
        out[i] = v
        cam[i] = cameras[i]
    return out, cam
