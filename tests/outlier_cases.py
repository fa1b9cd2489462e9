"""The outlier cloud (image_projection_node's /outlier_cloud, IP:300-303) stated on a chosen range image, and three more
images for it (tests/seg_cases.py builds the clouds): what tests/test_outlier_host.py checks the host call against and
tests/test_gpu_outlier.py / test_gpu_streams_map.py run on the device."""
import numpy as np

import seg_cases as sc

OUTLIER_MAX = (sc.ROWS - 6) * (sc.COLS // 5)


def yzx(cloud):
    """lins_streams_map_cloud's axes: (x, y, z) <- (y, z, x), intensity kept (SE:1128-1131)"""
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    return np.ascontiguousarray(c[:, [1, 2, 0, 3]])


def model_outlier_cells(img, model=None):
    """flat indices of the outlier cells a range image implies, in raster order: label invalid, row > 5, col % 5 == 0"""
    m = model if model is not None else sc.segment_model(img)
    lab = m["oracle_label"].ravel()
    flat = np.arange(sc.CELLS)
    return flat[(lab == 999999) & (flat // sc.COLS > 5) & (flat % sc.COLS % 5 == 0)]


def model_outlier_cloud(img, model=None):
    """the cloud itself: the cell-centre point cloud_from_range_image fires into each outlier cell, intensity =
    row + col / 10000 formed in double and rounded once (IP:234)"""
    cells = model_outlier_cells(img, model)
    p = sc.points_of(cells, np.asarray(img, np.float64).ravel()[cells])
    p[:, 3] = ((cells // sc.COLS).astype(np.float32).astype(np.float64) + (cells % sc.COLS).astype(np.float32).astype(np.float64) / 10000.0).astype(np.float32)
    return p


def no_outlier_image():
    """(a) one valid blob of 3 x 40 cells: nothing is an outlier"""
    img = np.zeros((sc.ROWS, sc.COLS))
    img[7:10, 100:140] = 10.0
    return img


def full_image():
    """(b) lone returns at every fifth column of rows 6 .. 15: exactly OUTLIER_MAX outliers.  Neighbouring columns are empty;
    the cell 255 columns on is populated too (255 = 5 * 51), so the range goes by (col / 5) mod 7 in steps of 3 % (51 mod 7
    = 2: never the same class; the connect limit along a row is a ratio of 1.00201), and rows alternate by a factor 1.25
    (limit between rows: 1.01954).  Columns beyond 1544 point at column 0: those of class 0 connect to it — a one-way edge
    into a cell that is its own seed, so every cell stays a segment of one."""
    img = np.zeros((sc.ROWS, sc.COLS))
    k = np.arange(sc.COLS // 5)
    for r in range(6, sc.ROWS):
        img[r, ::5] = 8.0 * 1.03 ** (k % 7) * 1.25 ** (r % 2)
    return img


EXTREME_CELLS = [(6, 0), (8, 40), (8, 45), (9, 0), (9, 1795), (11, 1795), (12, 0), (15, 1795)]


def extreme_image():
    """(c) outliers at the first and last qualifying cells, (6, 0) and (15, 1795), and small invalid segments: a line of
    8 cells in row 8 across the thread-run boundary at flat cell 14 442 = (8, 42) (outliers at columns 40 and 45: either
    side of it); a line that leaves row 9 at column 1799 and comes back in at column 0 (the right edge wraps inside the
    ring); and two lines that are neighbours in RASTER order across the end of ring 11 — (11, 1795 .. 1799) and
    (12, 0 .. 2) lie in one thread's run of 29 cells (21 576 .. 21 604)."""
    img = np.zeros((sc.ROWS, sc.COLS))
    img[6, 0] = img[15, 1795] = 10.0
    img[8, 38:46] = 10.0
    img[9, 1794:] = 10.0
    img[9, :2] = 10.0
    img[11, 1795:] = 12.0
    img[12, :3] = 15.0
    assert (8 * sc.COLS + 42) % sc.RUN == 0 and (11 * sc.COLS + 1795) // sc.RUN == (12 * sc.COLS + 2) // sc.RUN
    return img


IMAGES = {"no_outlier": no_outlier_image, "full": full_image, "extreme": extreme_image}
_BUILT = {}


def image_case(name):
    """dict(img, raw, model, cloud = the outlier cloud the model implies), built once per process (read-only)"""
    if name not in _BUILT:
        img = IMAGES[name]()
        model = sc.segment_model(img)
        raw = sc.cloud_from_range_image(img)
        raw.setflags(write=False)
        _BUILT[name] = dict(img=img, raw=raw, model=model, cloud=model_outlier_cloud(img, model))
    return _BUILT[name]
