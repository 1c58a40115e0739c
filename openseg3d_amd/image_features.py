"""Per-point image features on disk: the reference's pickled dict and a packed form the dataset reads without a pickle.

``ops.point_image_features`` (or its host twin) gives ``dense`` float32 [n, C] and ``camera`` int32 [n] for one frame;
the rows that hit a camera (``camera >= 0``) are what tools/extract_image_feature.py:99-102 stores.

dict file    ``<stem>.npy``: ``np.save`` of ``{row: float32 [C]}``, the reference's format (a pickle; loading it walks
             every row in Python).
packed file  ``<stem>.npz``: uncompressed, exactly two arrays -- ``rows`` int32 [K] ascending and ``feats`` float32 [K, C].
"""
import os

import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def to_packed(dense, camera):
    """-> (rows int32 [K] ascending, feats float32 [K, C]): the rows with a camera and their features."""
    dense, camera = _host(dense), _host(camera)
    if dense.ndim != 2 or dense.dtype != np.float32 or camera.shape != (dense.shape[0],):
        raise ValueError("to_packed: dense float32 [n, C] and camera [n] of one frame")
    rows = np.flatnonzero(camera >= 0).astype(np.int32)
    return rows, np.ascontiguousarray(dense[rows])


def to_dict(dense, camera):
    """-> the reference's ``point_image_features``: Python int row -> float32 [C], rows ascending
    (extract_image_feature.py:80-100).  Every value owns its memory, as the reference's slices of separate maps do not
    share one either once pickled."""
    rows, feats = to_packed(dense, camera)
    return {int(r): feats[j].copy() for j, r in enumerate(rows)}


def save_dict(path, dense, camera):
    """Write the reference's ``<name>.npy`` (extract_image_feature.py:102); returns the file's path."""
    path = path if path.endswith(".npy") else path + ".npy"
    np.save(path, to_dict(dense, camera), allow_pickle=True)
    return path


def save_packed(path, dense, camera):
    """Write ``<name>.npz`` with exactly the keys ``rows`` and ``feats``, uncompressed; returns the file's path."""
    path = path if path.endswith(".npz") else path + ".npz"
    rows, feats = to_packed(dense, camera)
    np.savez(path, rows=rows, feats=feats)
    return path


def load_packed(path):
    """``<name>.npz`` -> (rows, feats); never unpickles."""
    with np.load(path, allow_pickle=False) as z:
        if sorted(z.files) != ["feats", "rows"]:
            raise ValueError(f"{path}: a packed image-feature file holds exactly 'rows' and 'feats'")
        rows, feats = z["rows"], z["feats"]
    if rows.dtype != np.int32 or rows.ndim != 1 or feats.dtype != np.float32 or feats.ndim != 2 or len(feats) != len(rows):
        raise ValueError(f"{path}: rows int32 [K] and feats float32 [K, C] expected")
    return rows, feats


def load_dict(path, dim=None):
    """The reference's pickled dict -> (rows int32 [K] in the dict's order, feats float32 [K, dim])."""
    d = np.load(path, allow_pickle=True).item()
    rows = np.fromiter(d.keys(), dtype=np.int64, count=len(d)).astype(np.int32)
    if dim is None:
        dim = len(next(iter(d.values()))) if d else 0
    feats = np.zeros((len(d), dim), dtype=np.float32)
    for j, v in enumerate(d.values()):
        feats[j] = v
    return rows, feats


def load(stem, dim=None):
    """(rows, feats) from ``<stem>.npz`` if it exists, otherwise from ``<stem>.npy``; the packed file wins when both do."""
    if os.path.exists(stem + ".npz"):
        return load_packed(stem + ".npz")
    return load_dict(stem + ".npy", dim)
