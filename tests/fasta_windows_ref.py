"""The rule of `--from-fasta --windows` in plain Python ("--from-fasta --windows").  Two statements that
share no code: by_start enumerates the k-mer starts of a record's joined bytes (fasta_records_ref.joined) and puts each
counted k-mer into the windows that hold its first byte; by_slice is fasta_ref.count (oracle.count_fastq underneath) on
the record's extended slice `">x\\n" + J[wS : min(wS + N + k - 1, bases)]`.  They must agree on every case
(test_fasta_windows_rules.py), and the GPU (vk_count_fasta_windows_device) must equal both exactly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_records_ref as RR  # noqa: E402
import fasta_ref as FR  # noqa: E402

NO_WINDOW = 2 ** 64 - 1
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def nwin(bases, n, s):
    """Windows of a record of `bases` joined bytes: no partial ones."""
    return (bases - n) // s + 1 if bases >= n else 0


def by_start(record, k, n, s):
    """uint32 [nwin, 4^k]: every counted k-mer of the record goes to the windows whose [wS, wS + N) holds its start."""
    record = bytes(record)
    nw = nwin(len(record), n, s)
    out = np.zeros((nw, 4 ** k), dtype=np.uint32)
    for p in range(len(record) - k + 1):
        code = 0
        for b in record[p:p + k]:
            c = _CODE.get(b)
            if c is None:
                code = None
                break
            code = code * 4 + c
        if code is None:
            continue
        for w in range(max(0, (p - n) // s + 1), min(nw, p // s + 1)):   # wS <= p < wS + N
            out[w, code] += 1
    return out


def by_slice(record, k, n, s):
    """The same from the existing oracle: window w is the whole count of the sample `>x` + the window's extended slice."""
    record = bytes(record)
    nw = nwin(len(record), n, s)
    out = np.zeros((nw, 4 ** k), dtype=np.uint32)
    for w in range(nw):
        out[w] = FR.count(b">x\n" + record[w * s:min(w * s + n + k - 1, len(record))], k)[0]
    return out


def rows(data, k, n, s, counter=by_slice):
    """[uint32 [nwin_r, 4^k]] for every record of a sample (none for a bad start or an empty sample)."""
    return [counter(r, k, n, s) for r in RR.joined(data)]
