"""The lane-local device code of the assemblies' k-mer spectrum, run on the host (tests/emul/fasta_spectrum_emul.cpp
compiles the product's csrc/vk_fasta_spectrum.h) against tests/fasta_spectrum_ref.py: a lane at a time over every case, at
unit sizes 64, 256 and the default, the additions summed into a table equal to the rule's counts.  The sanitizer build is a
stand-alone program, run as a program, never loaded into python.  The emulation's header says what it does not cover (the
kernels' loads, scans and atomics: the GPU tests run those)."""
import functools

import pytest

import fasta_spectrum_cases as FC
import fasta_spectrum_emul_lib as EL
import fasta_spectrum_ref as FR

UNITS = (64, FC.SMALL_UNIT, FC.UNIT)


@functools.lru_cache(maxsize=None)
def expected(k, every):
    return [(name, text) + FR.spectrum_strings(text, k, every) for name, text in FC.cases(k)]


def check(name, got, row, status, counts):
    st, totals, table = got
    assert st == status, name
    if status:
        return
    assert totals[:4] == row[:4], name
    assert table == counts, name


@pytest.mark.parametrize("every", FC.EVERIES)
@pytest.mark.parametrize("k", FC.KS)
@pytest.mark.parametrize("unit", UNITS)
def test_emulation_equals_the_rule(unit, k, every):
    run = EL.load()
    for name, text, row, status, counts in expected(k, every):
        check(name, run(text, k, every, unit, FR.slots_for(len(text), 1)), row, status, counts)


def test_a_run_of_equal_keys_is_one_addition():
    """Poly-A unwrapped: every lane folds its 64 windows of the one key into one addition."""
    run = EL.load()
    k = 21
    text = dict(FC.cases(k))["poly_a_500_unwrapped"]
    st, totals, table = run(text, k, 1, FC.UNIT, 1024)
    assert st == 0 and table == {0: 500 - k + 1}
    lanes = -(-len(text) // FC.LANE)
    assert totals[4] <= lanes
    # a tandem repeat of period 7 has no two equal consecutive keys: an addition per window
    text = dict(FC.cases(k))["tandem_7"]
    st, totals, table = run(text, k, 1, FC.UNIT, 1024)
    assert totals[4] == totals[2] == sum(table.values())


def test_a_full_table_is_a_status_and_never_spins():
    run = EL.load()
    k = 21
    text = dict(FC.cases(k))["unwrapped_5_units"]   # more than 1,024 distinct keys
    want = FR.spectrum_strings(text, k, 1, slots=1024)
    assert want[1] == FR.VK_SPEC_TABLE_FULL
    st, totals, table = run(text, k, 1, FC.SMALL_UNIT, 1024)
    assert st == FR.VK_SPEC_TABLE_FULL and len(table) == 1024
    assert totals[3] == FR.spectrum_strings(text, k, 1)[0][FR.TAKEN]   # (taken windows are counted before the table is asked)


@pytest.mark.parametrize("k", FC.KS)
def test_emulation_under_address_and_undefined_sanitizers(tmp_path_factory, k):
    """No byte read before or past a sample, no probe past the table, no shift out of range, the same answers."""
    d = tmp_path_factory.mktemp("fasta_spectrum_emul")
    exe = EL.sanitizer_program(d)
    for every in FC.EVERIES:
        want = expected(k, every)
        for unit in (64, FC.SMALL_UNIT):
            got = EL.run_program(exe, d, [(text, k, every, FR.slots_for(len(text), 1)) for _, text, *_ in want], unit)
            for (name, _, row, status, counts), g in zip(want, got):
                check(name, g, row, status, counts)
