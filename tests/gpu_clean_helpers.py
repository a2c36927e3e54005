"""What the GPU tests of step B share (test_gpu_clean_edges.py, test_gpu_adapter_edges.py): a clean_cases batch into
HBM, through ImageEngine.clean, and the comparison with what the reference states per sample.  Tests only."""
import numpy as np


def upload(eng, b):
    """The batch's files in HBM, each with its slack right behind its end: (tensor, offsets, lengths of the files)."""
    slack = b.get("slack") or [b""] * len(b["texts"])
    dev, offs, _ = eng.upload([t + s for t, s in zip(b["texts"], slack)])
    assert not (offs % 16).any()
    return dev, offs, np.array([len(t) for t in b["texts"]], dtype=np.uint64)


def clean(eng, b, F, T, flags, adapters=None):
    """[(text, stats words, status[, adapter stats])] per sample as the GPU gives them; the padding is checked here."""
    dev, offs, lens = upload(eng, b)
    out, oo, ol, st, status, *rest = eng.clean(dev, offs, lens, b["records"], b["roles"], b["owner"], b["nsamples"],
                                               trim=(F, T), adapter=flags[0], merge=flags[1], dedup=flags[2],
                                               adapters=adapters)
    host = out.cpu().numpy()
    got = []
    for j in range(b["nsamples"]):
        o, n = int(oo[j]), int(ol[j])
        assert not host[o + n:o + (n + 15) // 16 * 16].any(), f"sample {j}: padding not zero"
        got.append((host[o:o + n].tobytes(), st[j].tolist(), int(status[j])) + tuple(r[j].tolist() for r in rest))
    return got


def same(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], f"sample {j}: status {g[2]}, expected {w[2]}"
        assert len(g[0]) == len(w[0]) and g[0] == w[0], f"sample {j}: {len(g[0])} bytes, expected {len(w[0])}"
        assert g[1] == w[1], f"sample {j}: stats"
        assert g[3:] == w[3:], f"sample {j}: adapter stats {g[3:]}, expected {w[3:]}"
