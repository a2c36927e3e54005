"""`--depth-filter LO:HI`: the band a read's median k-mer depth must lie in (ImageEngine.spectrum(depth=...),
include/vkimg.h VK_DEPTH_*), how a band given in multiples of a sample's k-mer coverage becomes two integers, and the
`"depth_filter"` object and stats.csv columns that state what the filter did.  The rule: INTEGRATION.md,
"`--depth-filter`: the rule".  Pure Python: everything here works from a row and the spectrum's estimates alone."""
import math
import re
from collections import namedtuple

from . import _capi

NSTAT, HIST_AT, BINS = _capi.VK_DEPTH_NSTAT, _capi.VK_DEPTH_HIST, 256
READS_IN, READS_KEPT, BASES_IN, BASES_KEPT, NO_WINDOWS = range(5)
OPEN = 2 ** 32 - 1          # an open upper end
UNFILTERED = (0, OPEN)      # the band of a sample whose band is not applied

# A band as given: each end None (open), an int (a multiplicity) or a float (a multiple of the sample's k-mer coverage).
Band = namedtuple("Band", "text lo hi")

_INT = re.compile(r"[0-9]+\Z")
_MULT = re.compile(r"([0-9]+(?:\.[0-9]*)?|\.[0-9]+)x\Z")


def _end(side, text):
    if side == "":
        return None
    if _INT.match(side):
        v = int(side)
        if v > OPEN:
            raise ValueError(f"{text}: a multiplicity is below 2^32")
        return v
    m = _MULT.match(side)
    if m:
        return float(m.group(1))
    raise ValueError(f"{text}: an end is a non-negative integer or a decimal followed by x (LO:HI, for example 2:40, :4 or 3x:)")


def parse_band(text):
    """`LO:HI` as a Band.  Either end may be empty, not both; an end is a non-negative integer below 2^32 or a decimal
    followed by `x`.  ValueError says what is wrong."""
    text = str(text).strip()
    if text.count(":") != 1:
        raise ValueError(f"{text}: a band is LO:HI (for example 2:40, :4 or 3x:)")
    lo, hi = (_end(side, text) for side in text.split(":"))
    if lo is None and hi is None:
        raise ValueError(f"{text}: a band has at least one end")
    if isinstance(lo, int) and isinstance(hi, int) and lo > hi:
        raise ValueError(f"{text}: LO is above HI")
    return Band(text, lo, hi)


def resolve(band, estimate):
    """(lo, hi, applied, reason) of a Band for a sample with these spectrum estimates (spectrum.estimate): integers
    stand as they are, `ax` as LO is ceil(a lambda) and `bx` as HI is floor(b lambda), lambda the sample's
    kmer_coverage, an open end is 0 or 2^32 - 1.  A band with an `x` end on a sample without an estimate is not applied --
    whole, its integer end included -- and neither is one that resolves to lo > hi (no depth lies in it): UNFILTERED,
    False and the reason."""
    lam = None
    if isinstance(band.lo, float) or isinstance(band.hi, float):
        lam = estimate.get("kmer_coverage")
        if estimate.get("reason") or lam is None:
            return UNFILTERED + (False, "no k-mer coverage estimate: " + str(estimate.get("reason")))
    lo = 0 if band.lo is None else band.lo if isinstance(band.lo, int) else math.ceil(band.lo * lam)
    hi = OPEN if band.hi is None else band.hi if isinstance(band.hi, int) else math.floor(band.hi * lam)
    lo, hi = min(int(lo), OPEN), min(int(hi), OPEN)
    if lo > hi:
        return UNFILTERED + (False, f"the band resolves to {lo}:{hi}, LO above HI")
    return lo, hi, True, None


def report(row, band, resolved, applied, reason):
    """The `"depth_filter"` object of `<sample>.spectrum.json`: row a VK_DEPTH_NSTAT row, band the Band as given,
    resolved = (lo, hi) as the kernel took them."""
    row = [int(x) for x in row]
    hist = row[HIST_AT:HIST_AT + BINS - 1]
    while hist and hist[-1] == 0:
        hist.pop()
    lo, hi = int(resolved[0]), int(resolved[1])
    return {"band": band.text, "lo": lo, "hi": None if hi == OPEN else hi, "applied": bool(applied), "reason": reason,
            "reads_in": row[READS_IN], "reads_kept": row[READS_KEPT], "bases_in": row[BASES_IN],
            "bases_kept": row[BASES_KEPT], "reads_without_windows": row[NO_WINDOWS],
            "median_depth_histogram": hist, "median_depth_255_and_more": row[HIST_AT + BINS - 1]}


def columns(row):
    """The stats.csv columns of a row."""
    return {"depth_reads_in": int(row[READS_IN]), "depth_reads_removed": int(row[READS_IN]) - int(row[READS_KEPT]),
            "depth_basepairs_removed": int(row[BASES_IN]) - int(row[BASES_KEPT])}
