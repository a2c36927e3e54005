"""Inputs of the `--from-fasta` tests: the CPU rules test (test_fasta_rules.py), the host emulation
(test_fasta_emulation.py) and the GPU tests (test_gpu_fasta.py) share them.  Every builder is deterministic and returns
a list of (name, FASTA bytes)."""
import numpy as np

KS = (5, 6, 7, 8, 9)
UNIT = 16384           # bytes of a unit of the kernel at its default (vk_fasta.h: kFaUnitBytes)
SPAN = 32 * UNIT       # bytes of a workgroup at its default
SMALL_UNIT = 256       # what the tests set VKIMG_FASTA_UNIT_BYTES to


def seq(seed, n, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def wrap(s, width, eol=b"\n", final=True):
    """s in lines of `width` bytes (None: one line), each ended by eol; final: also the last one."""
    if not s:
        return b""
    lines = [s] if width is None else [s[i:i + width] for i in range(0, len(s), width)]
    return eol.join(lines) + (eol if final else b"")


def fasta(recs, width, eol=b"\n", final=True):
    out = b""
    for i, (h, s) in enumerate(recs):
        last = i == len(recs) - 1
        out += b">" + h + eol + wrap(s, width, eol, final or not last)
    return out


def widths(k):
    return (1, 2, 3, k - 1, k, 60, 61, None)


def line_cases(k):
    recs = [(b"r1 first", seq(11, 203)), (b"r2", seq(12, 137)), (b"r3 short", seq(13, k - 1)), (b"r4", seq(14, k))]
    out = []
    for w in widths(k):
        out.append((f"width_{w}", fasta(recs, w)))
        out.append((f"width_{w}_crlf", fasta(recs, w, b"\r\n")))
        out.append((f"width_{w}_nofinal", fasta(recs, w, final=False)))
        out.append((f"width_{w}_crlf_nofinal_cr", fasta(recs, w, b"\r\n", final=False) + b"\r"))
    s = seq(15, 120)
    out.append(("empty_lines", b">e\n\n" + s[:30] + b"\n\n\n" + s[30:61] + b"\n\r\n\n" + s[61:] + b"\n\n"))
    out.append(("stray_cr", b">c\n" + s[:20] + b"\r" + s[20:40] + b"\n" + s[40:50] + b"\r\r\n" + s[50:70] + b"\r \n" + s[70:] + b"\n"))
    out.append(("cr_only_lines", b">c\r\n\r\n" + s[:33] + b"\r\n\r\n\r\n" + s[33:] + b"\r"))
    return out


def header_cases(k):
    s = seq(21, 150)
    return [
        ("acgt_header", b">ACGTACGTACGTTTGACCA ACGTACGTAAAC\n" + wrap(s, 60) + b">GGGGGGGGGGGGGGGGGGGG\n" + wrap(s[::-1], 60)),
        ("gt_in_header", b">a>b >>c>\n" + wrap(s, 60) + b">>\n" + wrap(s[:70], 60)),
        ("long_header", b">" + seq(22, 70000) + b"\n" + wrap(s, 60) + b">" + seq(23, 70000, b"ACGT>N ") + b"\n" + wrap(s[:90], 61)),
        ("no_sequence", b">only\n>two\n" + wrap(s, 60) + b">three\n"),
        ("header_only", b">nothing"),
        ("header_only_nl", b">nothing\n"),
        ("two_headers", b">one\n>two\n" + wrap(s, 60) + b">three\n>four\n" + wrap(s[:k], 60)),
        ("gt_in_sequence", b">r\n" + s[:40] + b">" + s[40:80] + b"\n" + s[80:100] + b">notaheader\n" + s[100:] + b"\n"),
        ("header_at_end_of_window", b">r\n" + s[:k - 1] + b"\n>x\n" + s[k - 1:2 * k] + b"\n>y\n" + s[:k] + b"\n>z\n" + s[:k - 1]),
    ]


def break_cases(k):
    s = seq(31, 400)
    a = s[:50] + b"N" + s[50:100] + b"N" * k + s[100:150] + b"n" + s[150:200]
    b = s.lower()[:100] + s[100:130] + b"RYKMSWBDHVN" + s[130:160].lower() + b"-*. \t" + s[160:200] + b"U" + s[200:230] + b"u@+"
    c = b"".join(s[10 * i:10 * i + (k - 1 if i % 2 else k)] + b"N" for i in range(30))
    return [
        ("n_runs", fasta([(b"n", a)], 60)),
        ("n_runs_w1", fasta([(b"n", a)], 1)),
        ("lower_iupac", fasta([(b"i", b)], 60)),
        ("lower_iupac_wk", fasta([(b"i", b)], k)),
        ("exact_runs", fasta([(b"x", c)], None)),
        ("exact_runs_w3", fasta([(b"x", c)], 3)),
        ("high_bytes", b">h\n" + s[:30] + bytes([0x80, 0xC1, 0xE1, 0xFF, 0x01, 0x00, 0x21, 0x61 ^ 0x80]) + s[30:60] + b"\n"),
    ]


def poly_a():
    """Poly-A of 1 MB in 60-column lines: every update hits one bin; a second record starts past the middle."""
    return [("poly_a", b">a\n" + wrap(b"A" * 600000, 60) + b">b poly\n" + wrap(b"A" * 400000, 60))]


def _tail(k):
    """What follows the swept header: sequence in short lines, a run of line ends, more sequence, a second header of
    100 bytes, a third record -- about 450 bytes that the sweep slides over every seam."""
    s = seq(41, 260)
    return (wrap(s[:40], 7) + b"\n\n\r\n\n\n\r\n" + wrap(s[40:120], k) + b">second ACGTACGT " + seq(42, 84) + b"\n" +
            wrap(s[120:200], 60, b"\r\n") + s[200:230] + b"N" + s[230:] + b"\n")


def seam_pads(unit):
    if unit <= 512:
        return list(range(0, unit + 65))
    near = list(range(0, 81)) + list(range(unit - 130, unit + 65))
    coarse = list(range(81, unit - 450, 509)) + list(range(unit - 450, unit - 130, 3))
    return sorted(set(near + coarse))


def seam_cases(k, unit):
    """One fixed text behind a header of 1 + pad + 1 bytes, pad sweeping 0..unit + 64."""
    t = _tail(k)
    return [(f"seam_{unit}_{p}", b">" + b"h" * p + b"\n" + t) for p in seam_pads(unit)]


def span_seam_cases(k):
    """The same text around the seam between two workgroups at the default unit (SPAN bytes)."""
    t = _tail(k)
    return [(f"span_{d}", b">" + b"h" * (SPAN + d - 2) + b"\n" + t) for d in (-300, -70, -3, -1, 0, 1)]


def batch_cases(k):
    """64 small samples whose lengths take every residue mod 16 (so does the padding behind each in the uploader's
    layout), among them an empty one and one that starts with '@'."""
    out = []
    for i in range(64):
        n = 16 * (i // 16) + i % 16 + (0 if i < 16 else 40)
        body = fasta([(b"s%d" % i, seq(100 + i, 300))], (1, 7, 60, None)[i % 4])
        out.append((f"batch_{i}", body[:n] if i < 32 else body[:200 + n]))
    out[5] = ("batch_empty", b"")
    out[37] = ("batch_fastq", b"@r1\n" + seq(7, 50) + b"\n+\n" + b"I" * 50 + b"\n")
    return out


def small_cases(k):
    return line_cases(k) + header_cases(k) + break_cases(k) + [("empty", b"")]


def all_cases(k):
    """Every case but the unit-sized sweeps (seam_cases at the default unit, span_seam_cases)."""
    return small_cases(k) + poly_a() + seam_cases(k, SMALL_UNIT) + batch_cases(k)
