"""`train` on the GPU: the batch kernel (vk_train_batch_device) against tests/train_ref.py, its argument checks, and
the command end to end -- train, then `query` with the files it wrote."""
import shutil
import warnings

import numpy as np
import pytest

import train_ref
from varkoder_amd import _capi, query
from varkoder_amd import train as T

pytestmark = pytest.mark.gpu

SHAPES = ((32, 32), (128, 128), (512, 512), (32, 224), (91, 224), (512, 224))

# B = 7 over a set of 5 images, so indices repeat.  Rows 0, 1, 2, 6 have neutral lighting; row 1 has lam == 1 and row 2
# is its own partner, so under MixUp and CutMix they take nothing from a partner; row 5 (lam == 0) is all partner.
IDX = np.array([0, 1, 2, 3, 4, 1, 3], dtype=np.uint32)
PARTNER = np.array([1, 0, 2, 4, 3, 6, 5], dtype=np.uint32)
LAM = np.array([0.3, 1.0, 0.6, 0.5, 0.9, 0.0, 0.75], dtype=np.float32)
BSHIFT = np.array([0, 0, 0, 0.4, -0.3, 0.2, 0], dtype=np.float32)
CSCALE = np.array([1, 1, 1, 1.2, 1, 0.8, 1], dtype=np.float32)


def image_set(side, n=5):
    """Seeded random images with the values 0 and 255 in plenty: the lighting step's clamp acts on them."""
    rng = np.random.default_rng(1000 + side)
    imgs = rng.integers(0, 256, (n, side, side), dtype=np.uint8)
    imgs[0, : side // 2] = 0
    imgs[1, : side // 2] = 255
    imgs[2, :, : side // 3] = 255
    imgs[3, side // 2:, side // 2:] = 0
    return imgs


_RESIZED = {}


def resized(side, out):
    """The float64 reference's input, computed once per shape and left unchanged."""
    if (side, out) not in _RESIZED:
        r = train_ref.resized_set(image_set(side), out)
        r.setflags(write=False)
        _RESIZED[(side, out)] = r
    return _RESIZED[(side, out)]


def f32_plain(r):
    """query.preprocess's float32 arithmetic on resized pixels: ((v / 255) - 0.5) / 0.5, three channels."""
    x = (r.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    return np.repeat(x[:, None], 3, axis=1)


def rect_for(out):
    return (out // 5 + 1, out // 7, out - out // 3 - 1, out - 2)   # odd corners, no multiple of four


def run_kernel(eng, dev, out, idx, partner, lam, bshift, cscale, rect, mode):
    return T.train_batch(eng, dev, idx, partner, lam, bshift, cscale, rect, mode, out_size=out).cpu().numpy()


@pytest.mark.parametrize("side,out", SHAPES)
def test_batch_kernel_against_the_float64_rule(engines, side, out):
    """Rows with neutral lighting that take no partner value: bit-identical to query.preprocess (fails on a tree without
    vk_train_batch_device).  Every other row: max abs error against the float64 restatement within four times the
    largest error of the float32 torch-CPU evaluation of the same formula on the same inputs (the factor covers the
    device's exp / log being a few ulp looser than the host's; observed values: DESIGN.md 4.11)."""
    import torch
    eng = engines(7)
    imgs = image_set(side)
    dev = torch.from_numpy(imgs).cuda()
    r = resized(side, out)
    plain = f32_plain(r)
    if side * out <= 160 * 1024 - 1024:   # (query.preprocess keeps its intermediate in LDS and refuses 512 x 512)
        assert np.array_equal(query.preprocess(eng, dev, out_size=out).cpu().numpy(), plain)
    cases = [(IDX, PARTNER, LAM, BSHIFT, CSCALE)]
    cases.append(tuple(np.array(a) for a in ([2], [0], [0.4], [0.3], [1.1])))     # B = 1, lit
    cases.append(tuple(np.array(a) for a in ([4], [0], [0.4], [0.0], [1.0])))     # B = 1, neutral
    for idx, partner, lam, bshift, cscale in cases:
        for mode in (0, 1, 2):
            rect = rect_for(out) if mode == 2 else (0, 0, 0, 0)
            args = (idx, partner, lam, bshift, cscale, rect, mode)
            got = run_kernel(eng, dev, out, *args)
            want = train_ref.batch_f64(r, *args)
            host = train_ref.batch_f32_torch(r, *args)
            assert got.shape == want.shape == (len(idx), 3, out, out) and got.dtype == np.float32
            exact = [i for i in range(len(idx)) if not train_ref.is_lit(bshift[i], cscale[i])
                     and not train_ref.takes_partner(i, partner, lam, rect, mode)]
            rest = [i for i in range(len(idx)) if i not in exact]
            for i in exact:
                assert np.array_equal(got[i], plain[idx[i]]), (mode, i)
            if len(idx) > 1:
                assert exact and rest
            if rest:
                host_err = np.abs(host[rest] - want[rest]).max()
                err = np.abs(got[rest] - want[rest]).max()
                print(f"side {side} out {out} B {len(idx)} mode {mode}: float32 host error {host_err:.3e}, kernel error {err:.3e}")
                assert host_err > 0.0
                assert err <= 4.0 * host_err, (mode, err, host_err)


@pytest.mark.parametrize("side,out", ((32, 32), (91, 224)))
def test_cutmix_edges(engines, side, out):
    """CutMix copies: inside the rectangle the partner row's value, outside the row's own, bit for bit -- for an empty
    rectangle, the whole image, one pixel, and rectangles flush with each border; the pixels just inside and just outside
    each corner are looked at one by one."""
    import torch
    eng = engines(7)
    dev = torch.from_numpy(image_set(side)).cuda()
    base = run_kernel(eng, dev, out, IDX, PARTNER, LAM, BSHIFT, CSCALE, (0, 0, 0, 0), 0)
    rects = [(5, 5, 5, 9), (0, 0, 0, 0), (3, 7, 9, 7), (0, 0, out, out), (7, 9, 8, 10), (0, 3, 5, 11), (out - 5, 3, out, 11),
             (3, 0, 11, 6), (3, out - 6, 11, out), (out - 1, out - 1, out, out), (0, 0, 1, 1), (1, 2, out - 3, out - 1)]
    for x1, y1, x2, y2 in rects:
        got = run_kernel(eng, dev, out, IDX, PARTNER, LAM, BSHIFT, CSCALE, (x1, y1, x2, y2), 2)
        inside = np.zeros((out, out), dtype=bool)
        inside[y1:y2, x1:x2] = True
        for i in range(len(IDX)):
            assert np.array_equal(got[i], np.where(inside, base[PARTNER[i]], base[i])), ((x1, y1, x2, y2), i)
        if x2 > x1 and y2 > y1:
            i, p = 0, int(PARTNER[0])
            for y, x, is_in in ((y1, x1, True), (y2 - 1, x2 - 1, True), (y1 - 1, x1, False), (y1, x1 - 1, False),
                                (y2, x2 - 1, False), (y2 - 1, x2, False)):
                if 0 <= y < out and 0 <= x < out:
                    assert got[i, 1, y, x] == (base[p, 1, y, x] if is_in else base[i, 1, y, x]), (x1, y1, x2, y2, y, x)


def test_argument_checks_refuse_on_the_host(engines):
    """Every refused input returns VK_EINVAL from the host-side validation and nothing is launched: the output keeps
    its sentinel."""
    import torch
    eng = engines(7)
    side, out = 32, 32
    dev = torch.from_numpy(image_set(side)).cuda()
    ok = dict(idx=IDX, partner=PARTNER, lam=LAM, bshift=BSHIFT, cscale=CSCALE, rect=(1, 2, 9, 9), mode=2, out_size=out)
    sentinel = torch.full((7, 3, out, out), -7.0, dtype=torch.float32, device="cuda")

    def bad(**change):
        kw = dict(ok, **change)
        with pytest.raises(_capi.VkError) as e:
            T.train_batch(eng, dev, out=sentinel, **kw)
        assert e.value.status == _capi.VK_EINVAL
        torch.cuda.synchronize()
        assert bool((sentinel == -7.0).all())
    bad(idx=np.array([0, 1, 2, 3, 5, 1, 3]))                        # idx == nset
    bad(partner=np.array([1, 0, 2, 4, 3, 7, 5]))                    # partner == B
    bad(lam=np.array([0.3, 1.0, 0.6, 0.5, 1.5, 0.0, 0.75]))
    bad(lam=np.array([0.3, 1.0, 0.6, 0.5, -0.1, 0.0, 0.75]))
    bad(lam=np.array([0.3, 1.0, np.nan, 0.5, 0.1, 0.0, 0.75]))
    bad(cscale=np.array([1, 1, np.inf, 1, 1, 1, 1]))
    bad(rect=(0, 0, out + 1, 4))
    bad(rect=(0, 0, 4, out + 1))
    bad(rect=(5, 0, 4, 4))
    bad(rect=(0, 5, 4, 4))
    bad(rect=(-1, 0, 4, 4))
    bad(mode=3)
    bad(std=0.0)
    # what vk_preprocess_device refuses: an intermediate that does not fit the LDS
    big = torch.zeros((1, 1024, 1024), dtype=torch.uint8, device="cuda")
    with pytest.raises(_capi.VkError) as e:
        T.train_batch(eng, big, [0], [0], [1.0], [0.0], [1.0], out_size=224)
    assert e.value.status == _capi.VK_EINVAL
    got = T.train_batch(eng, dev, out=sentinel, **ok)               # and the accepted call does run
    torch.cuda.synchronize()
    assert got is sentinel and not bool((sentinel == -7.0).any())


# ---- the command ---------------------------------------------------------------------------------------------------

EPOCHS_SINGLE, EPOCHS_MULTI = 4, 8


def make_toy_set(root, seed=7):
    """48 PNGs at k = 5 (32 x 32) of 12 samples in two classes: genus A is bright in the left half, genus B in the
    right, plus seeded noise; the labels go into the metadata."""
    from varkoder_amd.config import QUAL_THRESH
    from varkoder_amd.image import write_png
    rng = np.random.default_rng(seed)
    root.mkdir(parents=True, exist_ok=True)
    for s in range(12):
        cls = "A" if s % 2 == 0 else "B"
        for bp in (500, 1000, 2000, 5000):
            img = rng.integers(0, 96, (32, 32))
            img[:, :16] += 128 if cls == "A" else 0
            img[:, 16:] += 128 if cls == "B" else 0
            write_png(img.astype(np.uint8), root / f"s{s:02d}@{bp:08d}K+cgr+k5.png", [f"genus:{cls}", "family:F"], 0.001,
                      QUAL_THRESH, "cgr")
    return root


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return make_toy_set(tmp_path_factory.mktemp("train_toy") / "images")


def train_cli(toy, outdir, *flags):
    from varkoder_amd import cli
    args = cli.parse_args(["train", str(toy), str(outdir), "-c", "arias2022", "-R", "1", "-g"] + list(flags))
    with warnings.catch_warnings():   # (the label-mode warnings of check_label_types)
        warnings.simplefilter("ignore")
        return T.run_train(args)


@pytest.fixture(scope="module")
def single_run(toy, tmp_path_factory):
    out = tmp_path_factory.mktemp("train_single") / "model"
    return out, train_cli(toy, out, "-S", "-X", "None", "-p", "0", "-e", str(EPOCHS_SINGLE))


def held_out_folder(outdir, dest):
    import pandas as pd
    df = pd.read_csv(outdir / "input_data.csv")
    held = df[df["is_valid"]]
    assert 0 < len(held) < len(df)
    assert not set(held["sample"]) & set(df[~df["is_valid"]]["sample"])
    dest.mkdir(parents=True)
    for p in held["path"]:
        shutil.copyfile(p, dest / p.split("/")[-1])
    return held


def run_query(images, outdir, model_dir, *flags):
    import pandas as pd
    from varkoder_amd import cli
    cli.main(["query", "--images", "-l", str(model_dir / "trained_model.pt"), "--vocab", str(model_dir / "labels.txt"),
              "--input-size", "32"] + list(flags) + [str(images), str(outdir)])
    return pd.read_csv(outdir / "predictions.csv")


def test_train_then_query_single_label(toy, single_run, tmp_path):
    """`train -c arias2022 -S -X None -p 0 -R 1`, then `query --images` on the held-out images with the exported
    files: every held-out image gets its class.  Epochs: a CPU run of the same loop with train_ref's batch builder
    classified all 8 held-out images from epoch 1 on (lowest probability of the true class 0.994 after epoch 1, 1.000
    from epoch 2 on); 4 epochs are asked for."""
    outdir, history = single_run
    assert len(history) == EPOCHS_SINGLE and (outdir / "trained_model.pt").is_file()
    held = held_out_folder(outdir, tmp_path / "held")
    df = run_query(tmp_path / "held", tmp_path / "q", outdir, "--single-label")
    assert len(df) == len(held) == 8
    assert list(df["best_pred_label"]) == [T.sort_labels(x) for x in df["actual_labels"]]   # (-S joins the sorted labels)
    assert set(df["best_pred_label"]) == {"family:F;genus:A", "family:F;genus:B"}
    assert (outdir / "labels.txt").read_text().splitlines() == ["family:F;genus:A", "family:F;genus:B"]


def test_train_then_query_multilabel_defaults(toy, tmp_path):
    """The same with the default multilabel / MixUp / lighting settings: every held-out image's true labels are among
    the predictions at -d 0.5.  Epochs: the CPU run of the loop with train_ref's batch builder had every true label's
    probability above 0.5 on all 8 held-out images from epoch 1 on (lowest 0.742 after epoch 1, 0.995 after epoch 2, 1.000
    from epoch 3 on, no false label above 0.005 from there); 8 are asked for."""
    outdir = tmp_path / "model"
    history = train_cli(toy, outdir, "-e", str(EPOCHS_MULTI))
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    held_out_folder(outdir, tmp_path / "held")
    df = run_query(tmp_path / "held", tmp_path / "q", outdir, "-d", "0.5")
    assert (outdir / "labels.txt").read_text().splitlines() == ["family:F", "genus:A", "genus:B"]
    for truth, predicted in zip(df["actual_labels"], df["predicted_labels"].fillna("")):
        assert set(truth.split(";")) <= set(predicted.split(";")), (truth, predicted)


def test_same_seed_writes_the_same_tables_and_resume_starts_ahead(toy, single_run, tmp_path):
    """Two runs with the same -R write identical labels.txt and input_data.csv; and `-m trained_model.pt` starts from
    the earlier weights: its first-epoch validation loss is below a fresh model's."""
    flags = ("-S", "-X", "None", "-p", "0", "-e", "1")
    first = train_cli(toy, tmp_path / "a", *flags)
    second = train_cli(toy, tmp_path / "b", *flags)
    for name in ("labels.txt", "input_data.csv"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
        assert (tmp_path / "a" / name).read_bytes() == (single_run[0] / name).read_bytes(), name
    resumed = train_cli(toy, tmp_path / "c", "-m", str(single_run[0] / "trained_model.pt"), *flags)
    assert resumed[0]["valid_loss"] < first[0]["valid_loss"]
