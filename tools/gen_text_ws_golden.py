#!/usr/bin/env python3
"""tests/golden/text_ws.json: what the seven workspace-size functions of the record-text calls return, tabulated from a
library on a CPU (the size functions need no context).  The fixture that is committed was tabulated from the library of the
commit before the host rules moved into csrc/vk_textplan.h (VKIMG_LIB names the library to ask; default: the one in the
tree); tests/test_textplan_rules.py asks the header for every row.

Usage:  VKIMG_LIB=/path/to/libvkimg_hip.so python tools/gen_text_ws_golden.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import textplan_emul_lib as EM  # noqa: E402

CH, SB = EM.CHUNK, EM.SCAN_BLOCK
# a piece of u64 words takes one more 256-byte step for every 32 words: the scan's `sums` piece (blocks + 1 words) tells
# a layout sized for max(chunks, records) from one sized for the chunks only past 31 blocks
MANY = 32 * SB


def text_shapes():
    """(name, lengths, records) of the calls that index records."""
    shapes = [("none", [], [])]
    for ln in (0, 1, CH - 1, CH, CH + 1):
        for r in (0, 1, SB - 1, SB, SB + 1):
            shapes.append((f"one_len{ln}_rec{r}", [ln], [r]))
    shapes += [
        ("two", [CH + 1, 0], [1, 0]),
        ("two_budget_below", [1, CH], [SB + 1, 0]),
        ("three_empty_one_many", [0, 40, 3 * CH + 5], [0, 1, SB + 1]),
        ("three_even", [CH - 1, CH, CH + 1], [SB - 1, SB, SB + 1]),
        ("records_over_chunks", [100], [MANY]),            # 1 chunk, 32 scan blocks of records
        ("records_over_chunks_3", [0, 300, 100], [0, 7, MANY + 1]),
        ("chunks_over_records", [MANY * CH + 1], [5]),      # 32 scan blocks of chunks and one more chunk, 5 records
    ]
    return shapes


def rows(L):
    u64, u32 = C.c_uint64, C.c_uint32

    def arr(t, v):
        return (t * max(len(v), 1))(*v)

    def ask(fn, *args):
        out = u64()
        f = getattr(L, EM.SIZE_FNS[fn])
        f.restype = C.c_int
        st = f(*args, C.byref(out))
        assert st == 0, (EM.SIZE_FNS[fn], st)
        return int(out.value)

    out = []
    for name, lens, recs in text_shapes():
        n = u32(len(lens))
        a, r = arr(u64, lens), arr(u64, recs)
        for fn in (EM.SCREEN, EM.SPECTRUM, EM.DEPTH):
            out.append({"name": f"{EM.SIZE_FNS[fn]}:{name}", "fn": fn, "lengths": lens, "records": recs, "bytes": ask(fn, r, n, a)})
        out.append({"name": f"{EM.SIZE_FNS[EM.QC]}:{name}", "fn": EM.QC, "lengths": lens, "records": recs, "bytes": ask(EM.QC, r, a, n)})
    emit = [("no_steps", [CH + 1, 10], [3, 1], []),
            ("each_once", [CH + 1, 10], [3, 1], [0, 1]),
            ("one_twice", [CH + 1, 10], [SB, 1], [0, 0, 1]),
            ("out_of_range", [CH + 1, 10], [SB, 1], [0, 7]),        # (the step of sample 7 adds no items)
            ("no_samples_one_step", [], [], [0]),
            ("three_empty_one_many", [0, 40, 3 * CH + 5], [0, 1, SB + 1], [2, 1, 0, 2]),
            ("items_over_chunks", [100], [MANY // 2 + 1], [0, 0]),  # 1 chunk, 32 scan blocks of items and 2 more items
            ("chunks_over_items", [MANY * CH + 1], [5], [0])]
    for name, lens, recs, steps in emit:
        b = ask(EM.EMIT, arr(u64, recs), u32(len(lens)), arr(u64, lens), arr(u32, steps), u32(len(steps)))
        out.append({"name": f"{EM.SIZE_FNS[EM.EMIT]}:{name}", "fn": EM.EMIT, "lengths": lens, "records": recs, "step_sample": steps,
                    "bytes": b})
    for ln in (0, 63, 64, 65, 1 << 20):
        out.append({"name": f"{EM.SIZE_FNS[EM.SCREEN_BUILD]}:len{ln}", "fn": EM.SCREEN_BUILD, "length": ln,
                    "bytes": ask(EM.SCREEN_BUILD, u64(ln))})
    for name, lens in [("none", []), ("len0", [0]), ("len63", [63]), ("len64", [64]), ("len65", [65]), ("two", [65, 0]),
                       ("three", [63, 64, 1 << 20])]:
        out.append({"name": f"{EM.SIZE_FNS[EM.SPECTRUM_FASTA]}:{name}", "fn": EM.SPECTRUM_FASTA, "lengths": lens,
                    "bytes": ask(EM.SPECTRUM_FASTA, arr(u64, lens), u32(len(lens)))})
    return out


def main():
    path = os.environ.get("VKIMG_LIB") or os.path.join(ROOT, "varkoder_amd", "libvkimg_hip.so")
    doc = {"what": "the *_workspace_size results of the record-text calls, tabulated from the library before the host rules "
                   "moved into vk_textplan.h (tools/gen_text_ws_golden.py); fn indexes textplan_emul_lib.SIZE_FNS",
           "rows": rows(C.CDLL(path))}
    with open(os.path.join(ROOT, "tests", "golden", "text_ws.json"), "w") as f:
        f.write('{"what": %s,\n "rows": [\n' % json.dumps(doc["what"]))   # (a row a line)
        f.write(",\n".join("  " + json.dumps(r) for r in doc["rows"]) + "\n]}\n")
    print(len(doc["rows"]), "rows")


if __name__ == "__main__":
    main()
