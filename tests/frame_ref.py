"""Plain numpy restatements of the frame-assembly semantics (include/seg3d_hip.h, "Frame assembly"): the multi-sweep merge
of load_points / load_points_from_sweeps and the range-image loop of construct_seg_frame.  Shared by the host tests, the
GPU tests and tools/frame_bench.py."""
import numpy as np


def merge_sweeps(sweeps, matrices, lags, dim):
    """sweeps: raw [N_s, >= dim] arrays of one float dtype, current sweep first; matrices[s]: None or the 4 x 4 (3 x 4)
    float64 sensor-to-current-lidar matrix; lags[s]: the time-lag column.  Returns [sum N, dim] in the rows' dtype."""
    out = []
    for raw, m, lag in zip(sweeps, matrices, lags):
        p = np.array(raw[:, :dim])  # a copy in the rows' own dtype
        p[:, 3] = 0
        p[:, 4] = np.tanh(p[:, 4])
        if m is not None:
            m = np.asarray(m, dtype=np.float64)
            x, y, z = (p[:, k].astype(np.float64) for k in range(3))
            for k in range(3):
                prod = ((x * m[k, 0] + y * m[k, 1]) + z * m[k, 2]).astype(p.dtype)  # stored, then `+=`
                p[:, k] = (prod.astype(np.float64) + m[k, 3]).astype(p.dtype)
        p[:, 3] = lag
        out.append(p)
    return np.concatenate(out, axis=0)


def transform_bound(raw_xyz, m):
    """8 * 2^-53 * (|x||m0| + |y||m1| + |z||m2| + |t|) per coordinate: two evaluations of a three-term dot product differ
    by at most 2 * gamma_3, and the final add rounds once more in each."""
    m = np.abs(np.asarray(m, dtype=np.float64))
    return 8 * 2.0 ** -53 * (np.abs(raw_xyz.astype(np.float64)) @ m[:3, :3].T + m[:3, 3])


def range_images(pred, points_ri, rows=64, cols=2650):
    """construct_seg_frame's loop: channel 1 of image 1 / 2 at [row, col] = pred + 1 for return index 0 / 1; the last
    point wins; other return indices are skipped; an index outside the image raises IndexError."""
    img = [np.zeros((rows, cols, 2), dtype=np.int32), np.zeros((rows, cols, 2), dtype=np.int32)]
    for i in range(len(pred)):
        col, row, ret = (int(v) for v in points_ri[i])
        if ret not in (0, 1):
            continue
        if not (0 <= row < rows and 0 <= col < cols):
            raise IndexError(f"point {i}: ({row}, {col}) outside the {rows} x {cols} range image")
        img[ret][row, col, 1] = int(pred[i]) + 1
    return img[0], img[1]
