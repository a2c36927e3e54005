"""The k <= 7 count as resident workgroups that own samples and pull their chunks (vk_count.h, PullParams): every case bit
for bit against the oracle AND against the static launch of one workgroup per (sample, part) behind VKIMG_K1_STATIC=1,
for k = 5, 6, 7.  A chunk is the byte range of one wavefront of the static launch: chunk c of a sample is (part c // 16,
wave c % 16)."""
import numpy as np
import pytest

from fastq_cases import rec
from oracle import oracle
from varkoder_amd import synth

pytestmark = pytest.mark.gpu

KS = (5, 6, 7)
WAVES = 16    # kWaves
PIECE = 4096  # kPiece


@pytest.fixture(scope="module")
def engs():
    """get(k, mode): an engine whose k <= 7 count pulls ("pull", the default for samples of several parts; "pull0": samples of
    one part as well, with no helpers, VKIMG_K1_HELPERS=0) or is the static launch ("static")."""
    from varkoder_amd.engine import ImageEngine
    cache, mp = {}, pytest.MonkeyPatch()

    def get(k, mode):
        if (k, mode) not in cache:
            mp.delenv("VKIMG_K1_HELPERS", raising=False)
            if mode == "pull0":
                mp.setenv("VKIMG_K1_HELPERS", "0")
            if mode == "static":
                mp.setenv("VKIMG_K1_STATIC", "1")
            else:
                mp.delenv("VKIMG_K1_STATIC", raising=False)
            cache[(k, mode)] = ImageEngine(k=k, mapping="cgr", device=0)
            mp.delenv("VKIMG_K1_STATIC", raising=False)
            mp.delenv("VKIMG_K1_HELPERS", raising=False)
        return cache[(k, mode)]
    yield get
    for e in cache.values():
        e.close()
    mp.undo()


def resident_workgroups():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def chunks(length, parts):
    """[(w0, w1)] of the chunks of a sample that hold bytes (vk_count.h, wave_range)."""
    nblk = (length + 63) // 64
    bwg = (nblk + parts - 1) // parts
    bw = (bwg + WAVES - 1) // WAVES
    out = []
    for part in range(parts):
        for wave in range(WAVES):
            b0 = part * bwg + wave * bw
            b1 = min(part * bwg + min((wave + 1) * bw, bwg), nblk)
            if b0 < b1:
                out.append((b0 * 64, min(b1 * 64, length)))
    return out


def count_both(engs, k, samples, parts=0, twice=False, pull="pull"):
    """Counts the batch with the pulling and with the static launch, checks both against the oracle (histograms and
    status), and returns (helpers, flushes per sample, grid) of the pulling launch."""
    want = [oracle.count_fastq(bytes(s) if not isinstance(s, np.ndarray) else s, k) for s in samples]
    n, info = len(samples), None
    for mode in (pull, "static"):
        eng = engs(k, mode)
        dev, offs, lens = eng.upload(samples)
        for rep in range(2 if twice else 1):
            hist, status = eng.count(dev, offs, lens, parts=parts)
            got, st = hist.cpu().numpy().view(np.uint32), status.cpu().numpy()
            for i in range(n):
                assert int(st[i]) == want[i][2], (mode, rep, i)
                assert np.array_equal(got[i], want[i][0]), (mode, rep, i)
            helpers, flushes = eng.last_count_pull(n)
            if mode == pull:
                assert min(flushes) >= 1 and max(flushes) <= 1 + helpers, (rep, helpers, flushes)
                info = (helpers, flushes, eng.last_count_launch()["grid"])
            else:
                assert not any(flushes)
    return info


def plain(sample, reads, dist=0):
    return synth.sample_fastq(sample, reads, 150, dist=dist)


ONE_CHUNK = rec("r", "ACGTACGTTGCATTGACCA")                      # under 64 bytes: one chunk holds bytes
KWAVES_CHUNKS = b"".join(rec(f"q{i}", "ACGGTCATTGCAAGCTTAGCAGGATCCATG" * 4) for i in range(4))   # 992 bytes: 16 blocks of 64 bytes, one per chunk


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", ("one_chunk", "kwaves_chunks", "under_a_piece", "empty_among_others"))
def test_small_samples(engs, k, case):
    if case == "one_chunk":
        assert len(chunks(len(ONE_CHUNK), 1)) == 1
        samples = [ONE_CHUNK]
    elif case == "kwaves_chunks":
        assert len(chunks(len(KWAVES_CHUNKS), 1)) == WAVES
        samples = [KWAVES_CHUNKS]
    elif case == "under_a_piece":
        samples = [plain(3, 11)]   # 3520 bytes
        assert len(samples[0]) < PIECE
    else:
        samples = [plain(4, 300), b"", plain(5, 40), b"", ONE_CHUNK, plain(6, 700, dist=1)]
    helpers, flushes, grid = count_both(engs, k, samples, pull="pull0")   # (one part: pulled only with the bound forced)
    assert grid == len(samples) and helpers == 0   # samples of one part: an owner each
    if case == "empty_among_others":   # ... and by the rule, the static launch: no flush is counted
        eng = engs(k, "pull")
        dev, offs, lens = eng.upload(samples)
        eng.count(dev, offs, lens)
        assert eng.last_count_pull(len(samples)) == (0, [0] * len(samples))


@pytest.mark.parametrize("k", KS)
def test_fewer_samples_than_workgroups_are_helped_from_the_start(engs, k):
    samples = [plain(20 + i, 10000, dist=i % 2) for i in range(3)]   # 3.2 MB each: two parts, 32 chunks
    helpers, flushes, grid = count_both(engs, k, samples, twice=True)   # (twice: the cursors are zeroed again)
    assert helpers >= 1 and len(samples) < grid <= resident_workgroups()
    assert sum(flushes) > len(samples)   # somebody helped


@pytest.mark.parametrize("k", KS)
def test_more_samples_than_workgroups_owners_only(engs, k):
    samples = [plain(100 + i, 62, dist=i % 2) for i in range(600)]   # 19840 bytes each: one part, nobody to help
    helpers, flushes, grid = count_both(engs, k, samples, pull="pull0")
    assert helpers == 0 and flushes == [1] * len(samples)
    assert grid == min(len(samples), resident_workgroups())


@pytest.fixture(scope="module")
def one_big_among_small():
    return [plain(900, 125000)] + [plain(901 + i, 31, dist=i % 2) for i in range(200)]   # 40 MB, then 200 x 9920 bytes


@pytest.mark.parametrize("k", KS)
def test_one_big_sample_is_helped_within_the_bound(engs, k, one_big_among_small):
    samples = one_big_among_small
    helpers, flushes, grid = count_both(engs, k, samples)   # (count_both: 1 <= flushes <= 1 + helpers for every sample)
    assert helpers >= 1
    assert flushes[0] >= 2, "the big sample was finished by its owner alone"


# ---- chunk boundaries on every kind of line ----------------------------------------------------------------------

KINDS = ("header", "nl_header", "seq", "nl_seq", "plus", "nl_plus", "qual", "nl_qual")
STEER_LEN = 1310720          # 20480 blocks: with two parts 32 chunks of 40960 bytes (ten pieces)
STEER_CHUNK = 40960


def kind_at(d, n, hl):
    """What byte d of a record with a header line of hl bytes and a read of n bases is."""
    edges = ((hl, "header", "nl_header"), (hl + 1 + n, "seq", "nl_seq"), (hl + n + 3, "plus", "nl_plus"),
             (hl + 2 * n + 4, "qual", "nl_qual"))
    for at, inside, newline in edges:
        if d < at:
            return inside
        if d == at:
            return newline
    return None


def record(rng, n, hl):
    def text(alphabet, size):
        return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(len(alphabet), size=size)].tobytes().decode()
    name, seq, qual = text(b"abcdefgh0123456789:/ ", hl - 1), text(b"ACGT", n), text(b"@+I5#", n)
    if n:
        qual = "@+"[int(rng.integers(2))] + qual[1:]   # a quality line that opens like a header or a separator
    r = rec(name, seq, qual)
    assert len(r) == hl + 2 * n + 5
    return r


def steered_sample(seed):
    """Reads of 37, 150 and 290 bases under headers of 15 to 70 bytes, STEER_LEN bytes in all, laid out so that the chunk
    boundaries (multiples of STEER_CHUNK) fall on every kind of byte in turn."""
    rng = np.random.default_rng(seed)
    reads, hls = (37, 150, 290), range(15, 71)
    out, pos, nb = [], 0, 1

    def fit(d, want):
        for n in reads:
            for hl in hls:
                if kind_at(d, n, hl) == want:
                    return n, hl
        return None

    while STEER_LEN - pos >= 1500:
        d = nb * STEER_CHUNK - pos if nb * STEER_CHUNK < STEER_LEN else 1 << 30
        want = KINDS[(nb + seed) % len(KINDS)]
        if d > 1500:   # (far from the boundary; from here on short records walk up to it, so that no window is stepped over)
            n, hl = int(rng.choice(reads)), int(rng.integers(15, 71))
        else:
            got = fit(d, want)
            if got:
                n, hl = got
                nb += 1
            else:   # a short record after which the boundary is within reach
                n, hl = 37, next((h for h in hls if fit(d - (h + 2 * 37 + 5), want)), 15)
        out.append(record(rng, n, hl))
        pos += len(out[-1])
    left = STEER_LEN - pos
    hl = 15 if (left - 5 - 15) % 2 == 0 else 16
    out.append(record(rng, (left - 5 - hl) // 2, hl))
    data = b"".join(out)
    assert len(data) == STEER_LEN and nb == STEER_LEN // STEER_CHUNK
    return data


def byte_kinds(data):
    """kind of every byte of a four-line FASTQ text"""
    a = np.frombuffer(data, dtype=np.uint8)
    nl = a == 10
    line = np.concatenate(([0], np.cumsum(nl)[:-1])) & 3
    return np.where(nl, 1, 0) + 2 * line   # KINDS[...]: (header, nl_header, seq, nl_seq, ...)


@pytest.fixture(scope="module")
def boundary_samples():
    steered = [steered_sample(s) for s in range(3)]
    seen = set()
    for s in steered:
        kinds = byte_kinds(s)
        assert len(chunks(len(s), 2)) == 2 * WAVES
        seen |= {KINDS[int(kinds[w0])] for w0, _ in chunks(len(s), 2)[1:]}
    assert seen == set(KINDS), seen
    return steered + [synth.sample_fastq(40 + i, 4000, 150, dist=2) for i in range(3)]   # fastp-shaped: set-aside lists


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("parts", (0, 2))
def test_chunk_boundaries_on_every_kind_of_line(engs, k, parts, boundary_samples):
    # (parts 0: the rule gives these samples one part, 16 chunks each, pulled only with the bound forced)
    helpers, flushes, grid = count_both(engs, k, boundary_samples, parts=parts, pull="pull" if parts else "pull0")
    if parts == 2:
        assert grid == 2 * len(boundary_samples) and helpers == 1


@pytest.fixture(scope="module")
def edge_piece_samples():
    """A non-ASCII byte and a read rich in N in the first and in the last piece of a chunk: the general path at a chunk's edges."""
    out = []
    for s, what in enumerate(("nonascii", "nrich")):
        a = plain(60 + s, 4096).copy()   # 1310720 bytes as well: records of 320 bytes, sequence at 16 .. 166
        cs = chunks(len(a), 2)
        for c in (3, 17, 30):
            w0, w1 = cs[c]
            for at in (w0 + 1300, w1 - 1700):   # inside the first piece (it starts at w0 - 64), inside the last
                r = at // 320
                if what == "nonascii":
                    a[r * 320 + 169 + 7] = 0xC3   # in the quality line
                    a[(r + 1) * 320 + 5] = 0xA9   # in a header
                else:
                    a[r * 320 + 16:r * 320 + 166:3] = ord("N")
                    a[(r + 1) * 320 + 16 + 40:(r + 1) * 320 + 16 + 110] = ord("N")
        out.append(a)
    return out


@pytest.mark.parametrize("k", KS)
def test_general_path_at_chunk_edges(engs, k, edge_piece_samples):
    count_both(engs, k, edge_piece_samples, parts=2)
