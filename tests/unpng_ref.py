"""The PNG un-filter in numpy (PNG specification, filter method 0): the reference that the host emulation and the GPU
decoder are read against.  tests/test_unpng_ref.py checks it against PIL on every case file first."""
import numpy as np


def unpng_ref(raw, side):
    """The raw stream (side rows of a filter byte and side bytes) -> pixels [side, side] uint8.  Bytes outside the image
    count as 0, arithmetic is mod 256, Average is floor((left + up) / 2) on the 9-bit sum, Paeth breaks ties in the order
    left, up, up-left.  Raises ValueError for a stream of another length or a filter byte above 4."""
    if len(raw) != side * (side + 1):
        raise ValueError(f"{len(raw)} raw bytes, not {side * (side + 1)}")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(side, side + 1)
    out = np.zeros((side, side), dtype=np.uint8)
    up = np.zeros(side, dtype=np.int64)
    for r in range(side):
        ft, x = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 1:
            cur = np.cumsum(x) & 255   # a running sum mod 256
        elif ft == 2:
            cur = (x + up) & 255
        elif ft in (3, 4):
            cur = np.zeros(side, dtype=np.int64)
            a = c = 0
            for i in range(side):
                b = int(up[i])
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                a = cur[i] = (int(x[i]) + pred) & 255
                c = b
        else:
            raise ValueError(f"filter byte {ft} in row {r}")
        out[r] = cur
        up = cur
    return out
