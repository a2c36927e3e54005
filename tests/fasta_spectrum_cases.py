"""Named cases of `--genome-spectrum`, each a FASTA text of a few KB at most: what the rule tests
(test_fasta_spectrum_rules.py), the emulation (test_fasta_spectrum_emulation.py) and the GPU tests
(test_gpu_fasta_spectrum.py) share.  cases(k) is a list of (name, text); every builder is deterministic.  A lane of the
count kernel owns 64 bytes of text and a unit is 64 lanes at most (SMALL_UNIT: VKIMG_FASTA_UNIT_BYTES in the tests), so the
cases put line seams, headers and breaks at every phase of a lane and across units.  batch(k) is a batch with a bad start
and an empty sample between good ones; dense_taken() a larger text whose first table fills at every > 1."""
import functools
import random

from screen_cases import REFERENCE_CASES, fa, rc, seq

KS = (16, 21, 31)
EVERIES = (1, 4)
SMALL_UNIT, UNIT = 256, 16384
LANE = 64


def _pad_header(upto):
    """A header line of exactly `upto` bytes, its \\n included."""
    return b">" + b"h" * (upto - 2) + b"\n"


@functools.lru_cache(maxsize=None)
def cases(k):
    rng = random.Random(9000 + k)
    out = []
    body = seq(rng, 700)
    # line widths: seams at every phase of a 64-byte lane (width + 1 bytes a line); an unwrapped record of several units
    for width in (1, 59, 60, 64, 61):
        out.append(("width_%d" % width, fa([(b"w", body[:200] if width == 1 else body)], width)))
    out.append(("unwrapped_5_units", fa([(b"long", seq(rng, 5 * SMALL_UNIT + 37))], 1 << 20)))
    # line ends
    out.append(("crlf", fa([(b"a", body[:300]), (b"b", body[300:500])], 60, eol=b"\r\n")))
    out.append(("crlf_width_62", fa([(b"a", body[:400])], 62, eol=b"\r\n")))   # (\r and \n on either side of a lane's end)
    out.append(("no_final_newline", fa([(b"a", body[:333])], 60)[:-1]))
    out.append(("ends_in_cr", fa([(b"a", body[:333])], 60, eol=b"\r\n")[:-1]))
    out.append(("cr_inside_a_line", b">r\n" + body[:90] + b"\r" + body[90:200] + b"\n"))
    out.append(("blank_lines", fa([(b"r", body[:300])], 25).replace(b"\n", b"\n\n", 5)))
    # headers: one that begins in the middle of a lane, one on a lane's last byte, '>' alone, two in a row, one longer than
    # a unit, the text ending in a header
    first = _pad_header(10) + body[:2 * LANE + 30 - 10 - 1] + b"\n"          # the next header begins at byte 2 * 64 + 30
    out.append(("header_mid_lane", first + b">second\n" + body[200:400] + b"\n"))
    first = _pad_header(10) + body[:3 * LANE - 1 - 10 - 1] + b"\n"           # the next header begins at byte 3 * 64 - 1
    assert len(first) % LANE == LANE - 1
    out.append(("header_on_lane_last_byte", first + b">second\n" + body[200:400] + b"\n"))
    out.append(("header_gt_alone", b">\n" + body[:150] + b"\n>\n" + body[150:290] + b"\n"))
    out.append(("two_headers_in_a_row", b">a\n" + body[:100] + b"\n>empty\n>b\n" + body[100:220] + b"\n"))
    out.append(("header_longer_than_a_unit", b">a\n" + body[:100] + b"\n>" + b"ACGT" * (SMALL_UNIT // 4 + 9) + b"\n" + body[100:250] + b"\n"))
    out.append(("ends_in_header", b">a\n" + body[:130] + b"\n>last"))
    out.append(("ends_in_header_newline", b">a\n" + body[:130] + b"\n>last\n"))
    out.append(("header_only", b">nothing here\n"))
    out.append(("gt_inside_a_line", b">a\n" + body[:50] + b">" + body[50:120] + b"\n"))   # ('>' not at a line start: a non-base)
    # non-bases: N every K - 1, K and K + 1 bases; lower case and IUPAC bytes
    for step in (k - 1, k, k + 1):
        s = b"N".join(body[i:i + step] for i in range(0, 400, step))
        out.append(("n_every_%d" % step, fa([(b"n", s)], 60)))
    out.append(("lower_case", fa([(b"l", body[:300].lower())], 60)))
    out.append(("mixed_case", fa([(b"m", bytes(b | 0x20 if i % 3 else b for i, b in enumerate(body[:300])))], 61)))
    iupac = body[:80] + b"R" + body[80:160] + b"y" + body[160:240] + b"-" + body[240:300] + b"5*" + body[300:380]
    out.append(("iupac_and_others", fa([(b"i", iupac)], 60)))
    # keys: records of exactly K - 1 and K bases; a palindrome of even K = 16 (fw == rc, whatever k is counted); a record and
    # its reverse complement; poly-A of 500; a dinucleotide and a 7-base tandem repeat
    out.append(("k_minus_1_and_k", fa([(b"short", body[:k - 1]), (b"exact", body[100:100 + k]), (b"again", body[:k - 1])], 60)))
    half = seq(rng, 8)
    out.append(("palindrome_16", fa([(b"p", half + rc(half)), (b"q", seq(rng, 9) + half + rc(half) + seq(rng, 11))], 60)))
    out.append(("record_and_revcomp", fa([(b"f", body[:250]), (b"r", rc(body[:250]))], 60)))
    out.append(("poly_a_500", fa([(b"a", b"A" * 500)], 60)))
    out.append(("poly_a_500_unwrapped", fa([(b"a", b"A" * 500)], 1000)))
    out.append(("dinucleotide", fa([(b"d", b"AC" * 300)], 60)))
    out.append(("tandem_7", fa([(b"t", b"ACGGTCA" * 120)], 61)))
    out.append(("empty_text", b""))
    out.append(("bad_start", body[:100] + b"\n>late\n" + body[100:200] + b"\n"))
    # the screen's cases about a reference's text
    for c in REFERENCE_CASES:
        out.append(("screen_" + c.name, c.fasta))
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    assert max(len(t) for _, t in out) < 8192
    return out


@functools.lru_cache(maxsize=None)
def dense_taken(k, every, n, seed=5):
    """An unwrapped record of n bases in which far more than 1 / every of the windows have a taken key: each base is chosen,
    where one of the four does it, so that the window it completes is taken.  Selection is by key, so a table sized for a
    1 / every share of the text fills."""
    import spectrum_ref
    rng = random.Random(seed)
    mask = (1 << (2 * k)) - 1
    fw = rc_ = 0
    out = bytearray()
    for i in range(n):
        order = rng.sample(range(4), 4)
        pick = order[0]
        if i >= k - 1:
            for c in order:
                f, r = ((fw << 2) | c) & mask, (rc_ >> 2) | ((3 - c) << (2 * k - 2))
                if spectrum_ref.taken(min(f, r), every):
                    pick = c
                    break
        fw, rc_ = ((fw << 2) | pick) & mask, (rc_ >> 2) | ((3 - pick) << (2 * k - 2))
        out.append(b"ACGT"[pick])
    return fa([(b"dense", bytes(out))], 1 << 20)


def batch(k):
    """Samples of one call: good ones with a bad start and an empty sample between them."""
    by = dict(cases(k))
    return [("width_61", by["width_61"]), ("bad_start", by["bad_start"]), ("tandem_7", by["tandem_7"]), ("empty_text", b""),
            ("crlf", by["crlf"])]
