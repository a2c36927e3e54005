"""Inputs of the `--from-fasta --windows` tests: the CPU rules test (test_fasta_windows_rules.py), the host emulation
(test_fasta_windows_emulation.py) and the GPU tests (test_gpu_fasta_windows.py) share them.  Every builder is
deterministic and returns a list of (name, FASTA bytes).  The windows are short (N of 64 to 128 bases) so that texts of
a few KB hold many seams; UNITS are what the tests set VKIMG_FASTA_UNIT_BYTES to, so a span is one unit."""
import fasta_cases as FC

UNITS = (64, 128)
GEOMETRIES = ((100, 100), (96, 48), (96, 24), (64, 16), (576, 9))   # (N, S): m = 1, 2, 4, 4, 64 (S >= k for every k)
SEQ_N = b"ACGTACGTACGTN"


def seam_cases(n, s):
    """One record behind a header of 5..133 bytes, in one line: its first base moves over two units of 64, so every
    tile seam falls once in the middle of a lane, on a lane boundary and on a unit (= span) boundary; k-mers straddle
    every seam and complete in the next lane or unit."""
    out = []
    pads = list(range(3, 20)) + list(range(56, 70)) + [127, 128, 129, 131]
    for pad in pads if n < 200 else pads[::5]:   # (m = 64 takes long windows: fewer of the same)
        head = b">" + b"h" * pad + b"\n"
        out.append((f"seam_pad{pad}", head + FC.seq(pad, 3 * n + 2 * s + 7) + b"\n"))
    return out


def width_cases(n, s):
    """Line widths 60, 61 and 64 (a line end at every lane's last byte), and CRLF."""
    body = FC.seq(77, 4 * n + s + 11)
    out = [(f"width_{w}", b">w\n" + FC.wrap(body, w)) for w in (60, 61, 64)]
    out += [(f"width_{w}_crlf", b">w\r\n" + FC.wrap(body, w, b"\r\n")) for w in (60, 61, 64)]
    out.append(("width_60_nofinal", b">w\n" + FC.wrap(body, 60, final=False)))
    out.append(("stray_cr", b">c\n" + body[:n - 1] + b"\r" + body[n - 1:2 * n] + b"\r\r\n" + body[2 * n:] + b"\r"))
    return out


def break_cases(n, s):
    """A non-ACGT run across a seam (from 3 bytes before to 3 behind, and a long one over a whole tile), a header line
    inside a tile, poly-A over seams (a lane's folded addition is flushed at the seam)."""
    body = bytearray(FC.seq(78, 3 * n + s))
    for at in (s, 2 * s, n):
        body[at - 3:at + 3] = b"NNNNNN"
    long_run = bytearray(FC.seq(79, 3 * n + s))
    long_run[n - 5:n + s + 5] = b"N" * (s + 10)
    return [
        ("n_across_seams", b">n\n" + FC.wrap(bytes(body), 61)),
        ("n_over_a_tile", b">n\n" + FC.wrap(bytes(long_run), 60)),
        ("header_inside_a_tile", b">a\n" + FC.seq(80, n + s // 2) + b"\n>b mid tile\n" + FC.seq(81, 2 * n + 3) + b"\n"),
        ("poly_a", b">p\n" + FC.wrap(b"A" * (3 * n + 5), 60)),
        ("mixed_case_n", b">m\n" + FC.wrap(FC.seq(82, 3 * n, b"ACGTacgtN"), 61)),
    ]


def length_cases(n, s):
    """Records of exactly N - 1, N, N + S - 1, N + S bases; several records shorter than N in one lane between two long
    ones; empty records."""
    recs = [(b"len%d" % ln, FC.seq(90 + i, ln)) for i, ln in enumerate((n - 1, n, n + s - 1, n + s))]
    shorts = [(b"s%d" % i, FC.seq(95 + i, 4 + i)) for i in range(6)]
    return [
        ("exact_lengths", FC.fasta(recs, None)),
        ("exact_lengths_w61", FC.fasta(recs, 61)),
        ("shorts_between_longs", FC.fasta([(b"long1", FC.seq(96, 2 * n + 5))] + shorts + [(b"", b""), (b"long2", FC.seq(97, n + 2 * s + 1))], None)),
        ("shorts_between_longs_crlf", FC.fasta([(b"long1", FC.seq(96, 2 * n + 5))] + shorts + [(b"long2", FC.seq(97, n + 2 * s + 1))], 60, b"\r\n")),
    ]


def all_cases(n, s):
    return seam_cases(n, s) + width_cases(n, s) + break_cases(n, s) + length_cases(n, s)


def batch(n, s):
    """A batch: records of several lengths, a FASTQ (VK_ST_BAD_START), an empty sample, a header-only sample."""
    a = FC.fasta([(b"a%d" % i, FC.seq(400 + i, n + 37 * i)) for i in range(5)], 60)
    b = FC.fasta([(b"b0", FC.seq(410, 5 * n + 3, SEQ_N)), (b"b1", b""), (b"b2", FC.seq(411, 2 * n))], None)
    c = FC.fasta([(b"c%d" % i, FC.seq(420 + i, n + s * i + i)) for i in range(4)], 64, b"\r\n")
    return [("a", a), ("fastq", b"@r\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n"), ("b", b), ("empty", b""), ("header_only", b">x"), ("c", c)]
