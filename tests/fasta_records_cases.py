"""Inputs of the `--from-fasta --per-record` tests: the CPU rules test (test_fasta_records_rules.py), the host emulation
(test_fasta_records_emulation.py) and the GPU tests (test_gpu_fasta_records.py) share them.  Every builder is
deterministic and returns a list of (name, FASTA bytes); none depends on k (records of 4..9 bases cover k - 1 and k for
every k)."""
import fasta_cases as FC

UNIT, SPAN, SMALL_UNIT = FC.UNIT, FC.SPAN, FC.SMALL_UNIT
SECOND = b">second rec name\tx\n"   # the header that the sweeps move


def _around(first_len, tail=True):
    """A first record of first_len bytes in all (header, one sequence line), so that SECOND's '>' sits at first_len."""
    head = b">first one\n"
    body = FC.seq(first_len, first_len - len(head) - 1)
    out = head + body + b"\n" + SECOND + FC.wrap(FC.seq(61, 150), 60)
    if tail:
        out += b">third\r\n" + FC.wrap(FC.seq(62, 70), 33, b"\r\n")
    return out


def seam_cases_small():
    """SECOND's '>' at 20..340: every lane seam of two units of 256 bytes and the unit seams, in steps of one; its
    name (17 bytes) and the line end before it cross them too."""
    return [(f"seam_small_{p}", _around(p)) for p in range(20, 341)]


def seam_cases_default():
    """The same around a wave seam (4096), a unit seam (UNIT) and the seam between two workgroups (SPAN) at the default
    unit, in steps of one."""
    out = []
    for at in (4096, UNIT):
        out += [(f"seam_{at}_{d}", _around(at + d)) for d in range(-22, 5)]
    out += [(f"seam_span_{d}", _around(SPAN + d, tail=False)) for d in range(-20, 4)]
    return out


def _short_records():
    recs = [(b"", b"")] * 3 + [(b"a", b"A")]
    for n in range(4, 10):
        recs.append((b"len%d" % n, FC.seq(70 + n, n)))
        recs.append((b"len%d N" % n, FC.seq(80 + n, n - 1) + b"N" + FC.seq(90 + n, n)))
    return recs


def many_cases():
    """Many records in one lane: 32 empty records in 64 bytes; `>\\n`, `>a\\nA\\n`, records of 4..9 bases; names of 127,
    128 and 129 bytes; a name that crosses a unit seam at 256 and at UNIT; a header that is the sample's last line."""
    empty32 = b">\n" * 32
    short = FC.fasta(_short_records(), None)
    names = b"".join(b">" + FC.seq(30 + n, n, b"abcXYZ 09") + b"\n" + FC.seq(40 + n, 25) + b"\n" for n in (127, 128, 129))
    out = [
        ("empty32", empty32),
        ("empty32_then_sequence", empty32 + b">r\n" + FC.seq(1, 90) + b"\n" + empty32),
        ("short", short),
        ("short_crlf", FC.fasta(_short_records(), 5, b"\r\n")),
        ("names_127_128_129", names),
        ("names_crlf", names.replace(b"\n", b"\r\n")),
        ("last_header_no_newline", b">one\n" + FC.seq(2, 30) + b"\n>the last line"),
        ("last_header_cr", b">one\r\n" + FC.seq(2, 30) + b"\r\n>the last line\r"),
        ("only_header", b">alone"),
        ("two_in_a_row", b">one\n>two\n" + FC.seq(3, 40) + b"\n>three\n>four\n" + FC.seq(4, 9) + b"\n"),
        ("gt_in_sequence", b">r\n" + FC.seq(5, 40) + b">" + FC.seq(6, 40) + b"\nAC>not a header\n>yes\nACGTACGTACGT\n"),
        ("stray_cr", b">c\n" + FC.seq(7, 20) + b"\r" + FC.seq(8, 20) + b"\n>d\r\n\r\n" + FC.seq(9, 33) + b"\r\r\n>e\n" + FC.seq(10, 12) + b"\r"),
    ]
    for seam in (SMALL_UNIT, UNIT):
        for d in (-1, -9, -40):   # the name's '>' at seam + d, 60 bytes of name: it runs across the seam
            head = b">pad\n"
            pad = FC.seq(seam + d, seam + d - len(head) - 1)
            out.append((f"name_across_{seam}_{d}", head + pad + b"\n>" + FC.seq(11, 60, b"nameNAME_-.") + b"\n" + FC.seq(12, 77) + b"\n"))
    return out


def long_cases():
    """One record over many spans (2 MB: at the default unit every workgroup of it is on its LDS table for k <= 7) and
    300 short records behind it; the same wrapped at 60 columns with CRLF."""
    recs = [(b"chr1 a chromosome", FC.seq(100, 2000000, b"ACGTACGTACGTACGTN"))]
    recs += [(b"ctg%d len=%d" % (i, 30 + 7 * i), FC.seq(200 + i, 30 + 7 * i)) for i in range(300)]
    return [("long_unwrapped", FC.fasta(recs, None)), ("long_w60_crlf", FC.fasta(recs, 60, b"\r\n"))]


def carry_case():
    """100 KB of 40-base records: 400 units of 256 bytes, more than the scan kernel has threads."""
    recs = [(b"r%d" % i, FC.seq(300 + i, 40)) for i in range(2200)]
    return [("carry", FC.fasta(recs, None))]


def slot_batch():
    """Three samples of a few records each, for the slot selections."""
    a = FC.fasta([(b"a%d x" % i, FC.seq(400 + i, 150 + 90 * i)) for i in range(5)], 60)
    b = FC.fasta([(b"b0", FC.seq(410, 1200)), (b"b1", b""), (b"b2", FC.seq(411, 700, b"ACGTN"))], None)
    c = FC.fasta([(b"c%d" % i, FC.seq(420 + i, 333)) for i in range(4)], 70, b"\r\n")
    return [("slots_a", a), ("slots_b", b), ("slots_c", c)]


def batch_cases():
    """fasta_cases.batch_cases: 64 samples at every 16-byte residue with an empty one and a FASTQ (VK_ST_BAD_START,
    nrec = 0); here also a header-only file, and two samples of several records, among exact neighbours."""
    out = FC.batch_cases(7)
    out[9] = ("batch_header_only", b">nothing here")
    out[20] = ("batch_three", b">x\nACGTACGTAC\n>y\n>z\nTTTTTTTTTTTTGGGA\n")
    out[50] = ("batch_many", FC.fasta([(b"m%d" % i, FC.seq(500 + i, 20 + i)) for i in range(12)], 13))
    return out


def emulation_cases():
    return seam_cases_small()[::3] + many_cases() + slot_batch() + batch_cases()
