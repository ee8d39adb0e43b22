"""The two projection pictures of crate `oics` (packages/lib/src/transfer.rs:337-376, :409-455) restated for the tests,
numpy and plain Python only.  Input: a 2-D uint8 array of ANY values (neither function asks for a 0 / 255 image).

`horizontal_literal` / `vertical_literal` follow the Rust loops statement by statement -- the in-place writes of the
horizontal one and the HashMap grouping of the vertical one included.  `horizontal` / `vertical` are the closed forms
the kernels implement (csrc/projpic.hip):

  horizontal, row r:   k0 = index of the first pixel == 255 (cols when there is none), K = pixels != 255 (K >= k0);
                       columns [0, k0) keep the source bytes, [k0, K) are 0, [K, cols) are 255
  vertical, column c:  n = pixels <= 127; rows [0, rows - n) are 255, rows [rows - n, rows) are 0

tests/test_projpic_ref.py asserts that the two pairs agree, so the library is tested against the reference's loops."""
import numpy as np


def _u8c1(src):
    a = np.asarray(src)
    assert a.ndim == 2 and a.dtype == np.uint8, "8-bit, one channel"
    return a


def horizontal_literal(src):
    """transfer_thresh_binary_to_horizontal_projection, transfer.rs:337-376"""
    src = _u8c1(src)
    mat = src.copy()                              # :341  let mut mat = (&src.matrix).clone();
    for row_index in range(mat.shape[0]):         # :344  for row_index in 0..mat.rows()
        row = mat[row_index]                      # :346  mat.at_row_mut::<u8>(row_index)? -- a view: writes land in mat
        filled_index = 0                          # :348
        flag = False                              # :351
        for col_index in range(src.shape[1]):     # :354  for col_index in 0..src.matrix.cols()
            if row[col_index] == 255:             # :358  reads the row being written, not src
                flag = True                       # :359
                continue                          # :360
            if flag:                              # :367
                row[col_index] = 255              # :368
                row[filled_index] = 0             # :369
            filled_index += 1                     # :371
    return mat                                    # :375


def vertical_literal(src):
    """transfer_thresh_binary_to_vertical_projection, transfer.rs:409-455"""
    src = _u8c1(src)
    mat = src.copy()                                          # :413
    col_black_counts = {}                                     # :416  HashMap<i32, Vec<usize>>
    width, height = mat.shape[1], mat.shape[0]                # :418
    for col_index in range(width):                            # :421
        total = 0                                             # :422  let mut sum: i32 = 0;
        for row_index in range(height):                       # :425
            target = mat[row_index][col_index]                # :427
            if target <= 127:                                 # :428
                total += 1                                    # :429
            mat[row_index][col_index] = 255                   # :432
        col_black_counts.setdefault(total, []).append(col_index)  # :437-438  entry(sum).or_insert(vec![]).push(..)
    for counts, columns in col_black_counts.items():          # :442  (the HashMap's order: the writes do not overlap)
        for col_index in columns:                             # :444
            for row_index in range(height - counts, height):  # :446
                row = mat[row_index]                          # :447
                row[col_index] = 0                            # :449
    return mat                                                # :454


def horizontal(src):
    """the closed form of horizontal_literal, vectorised"""
    src = _u8c1(src)
    rows, cols = src.shape
    white = src == 255
    k0 = np.where(white.any(axis=1), white.argmax(axis=1), cols)[:, None]
    K = (cols - white.sum(axis=1))[:, None]
    c = np.arange(cols)[None, :]
    return np.where(c < k0, src, np.where(c < K, 0, 255)).astype(np.uint8)


def vertical(src):
    """the closed form of vertical_literal, vectorised"""
    src = _u8c1(src)
    rows = src.shape[0]
    n = (src <= 127).sum(axis=0)[None, :]
    r = np.arange(rows)[:, None]
    return np.where(r >= rows - n, 0, 255).astype(np.uint8)


# the three value classes of the tests: strictly 0 / 255, the predicates' edge values, any byte
VALUE_CLASSES = {"binary": (0, 255), "six": (0, 1, 127, 128, 254, 255), "any": None}


def random_image(rng, rows, cols, cls):
    """a rows x cols image of value class `cls`; about one in three is mostly white, as a sheet is"""
    vals = VALUE_CLASSES[cls]
    if vals is None:
        a = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    else:
        a = np.array(vals, np.uint8)[rng.integers(0, len(vals), (rows, cols))]
    if rng.random() < 0.35:
        a[rng.random((rows, cols)) < 0.7] = 255
    return a
