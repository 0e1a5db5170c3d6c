"""The metric rule of the frame codec (include/pcc.h) restated in numpy, float32 throughout.

forwards   q = rint((x - o) / v) per coordinate: one float32 subtraction, one correctly rounded float32 division,
           round-half-to-even; a row is VALID when its three coordinates are finite (the rows invalid="drop" keeps);
           a valid row whose q leaves [-32768, 32767] is off the grid.
backwards  x = o + t * v: one float32 multiplication, then one float32 addition; t = c at lod 0, and the centre of the
           cell's lattice points (c << k) + (2^k - 1) / 2 at lod k.
"""
import numpy as np

OFF_GRID, NON_FINITE = 1, 2


def _grid(voxel, origin):
    v = np.float32(voxel)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    assert np.isfinite(v) and v > 0 and np.isfinite(o).all()
    return v, o


def quantize(points, voxel, origin=(0.0, 0.0, 0.0)):
    """float32 [n, 3] -> (lattice int32 [n, 3], valid bool [n], status): lattice rows of invalid or off-grid rows are 0;
    status = OFF_GRID if a valid row is off the grid | NON_FINITE if a row is not valid"""
    p = np.asarray(points)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3
    v, o = _grid(voxel, origin)
    valid = np.isfinite(p).all(axis=1)
    with np.errstate(all="ignore"):
        q = np.rint((p - o) / v)
    assert q.dtype == np.float32
    on = ((q >= np.float32(-32768)) & (q <= np.float32(32767))).all(axis=1)      # on the float; False for NaN
    off = valid & ~on
    lattice = np.where((valid & on)[:, None], q, np.float32(0)).astype(np.int32)
    status = (OFF_GRID if off.any() else 0) | (NON_FINITE if (~valid).any() else 0)
    return lattice, valid, status


def centres(cells, lod):
    """t of the rule backwards, as float64 (exact): the lattice index, or the centre of the cell's lattice points"""
    c = np.asarray(cells).astype(np.int64)
    return (c * (1 << lod)).astype(np.float64) + ((1 << lod) - 1) / 2.0


def dequantize(cells, lod, voxel, origin=(0.0, 0.0, 0.0)):
    """int [m, 3] lattice points (lod 0) or cells of level of detail lod -> float32 [m, 3]"""
    v, o = _grid(voxel, origin)
    t = centres(cells, lod)
    t32 = t.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t)      # a half-integer below 2^16: exact in float32
    x = o + t32 * v
    assert x.dtype == np.float32
    return x.reshape(-1, 3)
