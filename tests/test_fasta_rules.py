"""`--from-fasta` without a GPU: the rule's two statements agree on every case the GPU tests use (fasta_ref's
conversion + oracle.count_fastq against the brute-force walk, k = 5..9); the listing and naming of the input folder; the
refused flag combinations; and the namespaces of the command lines from before the flag, which must not change."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ref as FR  # noqa: E402

_WALKED = {}


def walked(data):
    if data not in _WALKED:
        _WALKED[data] = FR.brute_stretches(data)
    return _WALKED[data]


@pytest.mark.parametrize("k", FC.KS)
def test_the_two_statements_of_the_rule_agree(k):
    cases = FC.all_cases(k) + FC.seam_cases(k, FC.UNIT)[::16] + FC.span_seam_cases(k)[:1]
    assert len({name for name, _ in cases}) == len(cases)
    some = 0
    for name, data in cases:
        hist, st, nb = FR.count(data, k)
        if st:
            assert data[:1] != b">" and not hist.any() and nb == 0, name
            continue
        bh, bnb = FR.brute_count(data, k, walked(data))
        assert nb == bnb, name
        assert bh.max(initial=0) < 2 ** 32 and np.array_equal(hist.astype(np.uint64), bh), name
        some += int(bh.sum())
    assert some > 1000000


def test_known_answers():
    """First principles, k = 5: windows run across line ends, not across records, other bytes or header text."""
    k = 5

    def codes(data):
        return {FR_kmer(c, k): int(n) for c, n in enumerate(FR.count(data, k)[0]) if n}

    def FR_kmer(c, k):
        return "".join("ACGT"[(c >> (2 * (k - 1 - i))) & 3] for i in range(k))

    assert codes(b">r\nACG\nTA\n") == {"ACGTA": 1}
    assert codes(b">r\nACG\r\nTA\r") == {"ACGTA": 1}
    assert codes(b">r\nACG\n>ACGTACGT\nTA\n") == {}
    assert codes(b">r\nACGNTACGT\n") == {"TACGT": 1}
    assert codes(b">r\nAC\rGTA\n") == {}
    assert codes(b">r\nacg\n\n\nta>\n") == {"ACGTA": 1}
    assert codes(b">r\nAC>GTACG\n") == {"GTACG": 1}
    assert FR.count(b">r\nAC\r\nG T\r", k)[2] == 5 and FR.count(b">r\nAC\rG\n", k)[2] == 4
    assert FR.count(b"", k)[1:] == (0, 0) and FR.count(b"@r\nACGTA\n+\nIIIII\n", k)[1] == FR.VK_ST_BAD_START
    assert FR.to_fastq(b">a\n>b x\nAC\nGT\n>c\n") == b"@r1\nACGT\n+\nIIII\n"


def test_listing_and_naming(tmp_path):
    from varkoder_amd.fasta import fasta_files, image_name, sample_of
    names = ["b.fa", "a.fasta.gz", "c.v2.fna", "d.fa.gz", "e.fna.gz", "f.fasta", "notes.txt", "g.fq", "h.fa.bak", ".fa", "i.gz"]
    for n in names:
        (tmp_path / n).write_bytes(b">x\nACGT\n")
    (tmp_path / "sub.fa").mkdir()
    files = fasta_files(tmp_path)
    assert [f.name for f in files] == ["a.fasta.gz", "b.fa", "c.v2.fna", "d.fa.gz", "e.fna.gz", "f.fasta"]
    assert [sample_of(f) for f in files] == ["a", "b", "c.v2", "d", "e", "f"]
    assert sample_of("x/g.fq") is None and sample_of("h.fa.bak") is None and sample_of(".fa") is None
    assert image_name("a", 16569, 7, "cgr") == "a@00000016K+cgr+k7.png"
    assert image_name("c.v2", 999, 9, "varKode") == "c.v2@00000000K+varKode+k9.png"
    (tmp_path / "b.fasta").write_bytes(b">x\n")
    with pytest.raises(Exception, match="Two FASTA files for sample b"):
        fasta_files(tmp_path)


@pytest.mark.parametrize("argv", (
    ["image", "d", "--from-fasta", "--write-splits", "-i", "int"],
    ["image", "d", "--from-fasta", "--gpu-gzip"],
    ["image", "d", "--from-fasta", "--gpu-gzip", "-i", "int"],
    ["image", "d", "--from-fasta", "--from-raw"],
    ["image", "d", "--from-fasta", "--from-clean"],
    ["image", "d", "--from-fasta", "--detect-adapters"],
    ["query", "d", "o", "-l", "m", "--vocab", "v", "--from-fasta", "--images"],
    ["query", "d", "o", "-l", "m", "--vocab", "v", "--from-fasta", "--from-raw"],
    ["query", "d", "o", "-l", "m", "--vocab", "v", "--from-fasta", "--gpu-gzip"],
))
def test_refused_combinations_exit_2(argv, capsys):
    from varkoder_amd.cli import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_the_flag_parses_and_old_command_lines_keep_their_namespaces():
    from varkoder_amd.cli import parse_args
    a = parse_args(["image", "d", "--from-fasta", "-k", "9", "-t", "--labels-csv", "l.csv"])
    assert a.from_fasta is True and not a.from_raw and not a.from_clean and a.kmer_size == 9
    q = parse_args(["query", "d", "o", "-l", "m", "--vocab", "v", "--from-fasta"])
    assert q.from_fasta is True and not q.from_raw and not q.images
    image_keys = {"command", "input", "seed", "overwrite", "verbose", "kmer_size", "kmer_mapping", "n_threads",
                  "cpus_per_thread", "outdir", "stats_file", "int_folder", "min_bp", "max_bp", "label_table", "no_adapter",
                  "no_deduplicate", "no_merge", "no_image", "trim_bp", "labels_csv", "from_clean", "from_raw"}
    query_keys = {"command", "input", "outdir", "seed", "overwrite", "verbose", "model", "vocab", "single_label", "input_size",
                  "half", "no_pairs", "images", "kmer_size", "kmer_mapping", "n_threads", "cpus_per_thread", "stats_file",
                  "threshold", "int_folder", "keep_images", "include_probs", "no_adapter", "no_merge", "no_deduplicate",
                  "trim_bp", "max_bp", "from_raw", "max_batch_size"}
    for argv, extra in ((["image", "d"], set()), (["image", "d", "--from-clean"], set()), (["image", "d", "--from-raw"], set()),
                        (["image", "d", "--from-raw", "-i", "int", "--write-splits", "--gpu-gzip"], {"write_splits", "gpu_gzip"}),
                        (["image", "d", "--from-raw", "--detect-adapters"], {"detect_adapters"})):
        got = vars(parse_args(argv))
        assert set(got) == image_keys | extra, argv
        assert (got["kmer_size"], got["kmer_mapping"], got["min_bp"], got["max_bp"], got["outdir"], got["stats_file"],
                got["trim_bp"], got["n_threads"]) == (7, "cgr", "500K", "200M", "images", "stats.csv", "10,10", 1), argv
    for argv in (["query", "d", "o", "-l", "m", "--vocab", "v"], ["query", "d", "o", "-l", "m", "--vocab", "v", "--from-raw"],
                 ["query", "d", "o", "-l", "m", "--vocab", "v", "-I"]):
        got = vars(parse_args(argv))
        assert set(got) == query_keys, argv
        assert (got["kmer_size"], got["kmer_mapping"], got["max_bp"], got["threshold"], got["max_batch_size"],
                got["input_size"]) == (7, "cgr", "200M", 0.7, 64, 224), argv
    for argv in (["convert", "cgr", "i", "o"], ["train", "i", "o"]):
        assert "from_fasta" not in vars(parse_args(argv))
