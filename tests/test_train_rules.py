"""The host side of `train` (varkoder_amd/train.py): augmentation draws, batch size, validation split, vocabulary and
targets, the asymmetric loss, the command line and the exported model files.  No GPU."""
import warnings

import numpy as np
import pytest

import train_ref
from varkoder_amd import _capi, cli
from varkoder_amd import train as T


def gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


# ---- draw_batch_params ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1, 2))
def test_same_seed_same_arrays(mode):
    a = T.draw_batch_params(gen(5), 16, 224, mode, 0.75, 0.25)
    b = T.draw_batch_params(gen(5), 16, 224, mode, 0.75, 0.25)
    c = T.draw_batch_params(gen(6), 16, 224, mode, 0.75, 0.25)
    for k in ("partner", "lam", "bshift", "cscale"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) and a[k].shape == (16,)
    assert a["rect"] == b["rect"]
    assert not np.array_equal(a["bshift"], c["bshift"])
    assert a["partner"].dtype == np.uint32 and a["lam"].dtype == a["bshift"].dtype == a["cscale"].dtype == np.float32


def test_lighting_draws():
    for p, l in ((0.0, 0.25), (0.75, 0.0)):
        d = T.draw_batch_params(gen(1), 64, 32, 1, p, l)
        assert not d["bshift"].any() and (d["cscale"] == 1.0).all()
    l = 0.25
    d = T.draw_batch_params(gen(2), 4096, 32, 0, 0.75, l)
    lit_b, lit_c = d["bshift"] != 0, d["cscale"] != 1
    assert 0.70 < lit_b.mean() < 0.80 and 0.70 < lit_c.mean() < 0.80
    assert 0.50 < (lit_b & lit_c).mean() < 0.62                     # independent: 0.5625
    b = 1.0 / (1.0 + np.exp(-d["bshift"][lit_b].astype(np.float64)))
    assert b.min() >= 0.5 * (1 - l) - 1e-6 and b.max() <= 0.5 * (1 + l) + 1e-6
    c = d["cscale"][lit_c]
    assert c.min() >= 1 - l - 1e-6 and c.max() <= 1 / (1 - l) + 1e-6 and c.min() < 0.8 and c.max() > 1.25
    d = T.draw_batch_params(gen(2), 64, 32, 0, 1.0, l)
    assert (d["partner"] == np.arange(64)).all() and (d["lam"] == 1.0).all() and d["rect"] == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        T.draw_batch_params(gen(2), 4, 32, 0, 1.0, 1.0)
    with pytest.raises(ValueError):
        T.draw_batch_params(gen(2), 4, 32, 3, 1.0, 0.1)


def test_mixup_draws():
    d = T.draw_batch_params(gen(3), 512, 32, 1, 0.75, 0.25)
    assert (d["lam"] >= 0.5).all() and (d["lam"] <= 1.0).all() and d["lam"].std() > 0.05
    assert sorted(d["partner"].tolist()) == list(range(512)) and (d["partner"] != np.arange(512)).any()
    assert d["rect"] == (0, 0, 0, 0)


def test_cutmix_draws():
    out = 224
    areas = []
    for seed in range(40):
        d = T.draw_batch_params(gen(seed), 8, out, 2, 0.75, 0.25)
        x1, y1, x2, y2 = d["rect"]
        assert 0 <= x1 <= x2 <= out and 0 <= y1 <= y2 <= out
        assert np.allclose(d["lam"], 1.0 - (x2 - x1) * (y2 - y1) / out ** 2, atol=1e-7) and len(set(d["lam"].tolist())) == 1
        assert sorted(d["partner"].tolist()) == list(range(8))
        areas.append((x2 - x1) * (y2 - y1))
    assert len(set(areas)) > 20
    for t in (0.0, 1e-12, 1e-6, 0.5, 1.0 - 1e-6, 1.0 - 1e-12, 1.0):   # t near 0: the whole image; near 1: nothing
        for cx, cy in ((0, 0), (out - 1, out - 1), (0, out - 1), (out // 2, out // 3), (out - 1, 0)):
            x1, y1, x2, y2, lam = T.cutmix_rect(t, cx, cy, out)
            assert 0 <= x1 <= x2 <= out and 0 <= y1 <= y2 <= out and 0.0 <= lam <= 1.0
            assert lam == 1.0 - (x2 - x1) * (y2 - y1) / out ** 2
    assert T.cutmix_rect(0.0, out // 2, out // 2, out) == (0, 0, out, out, 0.0)
    assert T.cutmix_rect(1.0, 5, 5, out)[4] == 1.0


def test_batch_size_rule():
    assert [T.batch_size(n) for n in (1, 7, 10, 640, 100000)] == [1, 1, 1, 64, 64]
    assert T.batch_size(100000, 1, 4096) == 4096 and T.batch_size(100000, 1, 1 << 20) == 8192
    assert T.batch_size(7, 8, 64) == 8 and T.batch_size(160, 1, 64) == 16 and T.batch_size(640, 1, 32) == 32
    assert isinstance(T.batch_size(1), int)


# ---- split, vocabulary, targets ------------------------------------------------------------------------------------

def frame():
    import pandas as pd
    rows = []
    for s in range(23):
        labels = ("b;a", "c", "a;b", "d")[0 if s < 10 else 1 if s < 20 else 2 if s < 22 else 3]
        for bp in (1, 2, 3):
            rows.append({"sample": f"s{s:02d}", "bp": bp * 1000, "path": f"s{s:02d}@{bp}K+cgr+k7.png", "labels": labels})
    return pd.DataFrame(rows)


def test_random_split_is_by_sample_and_per_label_combination():
    df = T.validation_split(frame(), None, 0.2, seed=4)
    assert set(df["labels"]) == {"a;b", "c", "d"}                               # sorted within a row
    held, kept = set(df[df["is_valid"]]["sample"]), set(df[~df["is_valid"]]["sample"])
    assert not held & kept and len(held) + len(kept) == 23
    per = df[df["is_valid"]].drop_duplicates("sample").groupby("labels").size().to_dict()
    assert per == {"a;b": 2, "c": 2}            # 12 and 10 samples at 0.2 (round); the one `d` sample (< 1 / f) stays
    again = T.validation_split(frame(), None, 0.2, seed=4)
    assert list(again["is_valid"]) == list(df["is_valid"])
    other = T.validation_split(frame(), None, 0.2, seed=5)
    assert list(other["is_valid"]) != list(df["is_valid"])
    half = T.validation_split(frame(), None, 0.5, seed=4)
    assert half[half["is_valid"]].drop_duplicates("sample").groupby("labels").size().to_dict() == {"a;b": 6, "c": 5}


def test_given_validation_set(tmp_path):
    want = {"s01", "s15", "s22"}
    df = T.validation_split(frame(), "s01,s15,s22")
    assert set(df[df["is_valid"]]["sample"]) == want and df["is_valid"].sum() == 9
    (tmp_path / "v.txt").write_text("s01,s15,s22\n")
    df2 = T.validation_split(frame(), str(tmp_path / "v.txt"))
    assert list(df2["is_valid"]) == list(df["is_valid"]) and set(df2["labels"]) == {"a;b", "c", "d"}


def test_vocabulary_and_targets():
    df = T.validation_split(frame(), "s01")
    assert T.vocabulary(df, False) == ["a", "b", "c", "d"]
    y = T.targets(df, ["a", "b", "c", "d"], False)
    assert y.dtype == np.float32 and y.shape == (69, 4)
    assert y[0].tolist() == [1, 1, 0, 0] and y[30].tolist() == [0, 0, 1, 0] and y[68].tolist() == [0, 0, 0, 1]
    assert T.vocabulary(df, True) == ["a;b", "c", "d"]
    y = T.targets(df, ["a;b", "c", "d"], True)
    assert y.dtype == np.int64 and y[0] == 0 and y[30] == 1 and y[60] == 0 and y[68] == 2


def test_label_type_warnings():
    df = T.validation_split(frame(), "s01")
    with pytest.warns(UserWarning, match="multilabel model instead"):
        T.check_label_types(df, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.check_label_types(df, False)
    with pytest.warns(UserWarning, match="single label model instead"):
        T.check_label_types(df[df["labels"] == "c"], False)


def test_collect_images_reads_names_chunks_and_tables(tmp_path):
    from varkoder_amd.image import write_png
    rng = np.random.default_rng(0)
    (tmp_path / "in" / "sub").mkdir(parents=True)
    for s, labels, sd in (("x1", ["g:a", "f:b"], 0.001), ("x2", ["g:c"], 0.5)):
        write_png(rng.integers(0, 256, (32, 32), dtype=np.uint8), tmp_path / "in" / "sub" / f"{s}@00000500K+cgr+k5.png", labels,
                  sd, 0.01, "cgr")
    df = T.collect_images(tmp_path / "in")
    assert list(df.columns) == ["sample", "bp", "img_kmer_mapping", "img_kmer_size", "path", "labels", "possible_low_quality"]
    assert list(df["sample"]) == ["x1", "x2"] and list(df["labels"]) == ["g:a;f:b", "g:c"] and list(df["bp"]) == [500000] * 2
    (tmp_path / "t.csv").write_text("sample,labels,other\nx2,q;r,1\nx9,z,2\n")
    df = T.collect_images(tmp_path / "in", tmp_path / "t.csv")
    assert list(df["sample"]) == ["x2"] and list(df["labels"]) == ["q;r"]


# ---- loss ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma_neg", (0.0, 2.0, 4.0))
def test_asymmetric_loss_against_float64(gamma_neg):
    import torch
    rng = np.random.default_rng(int(gamma_neg))
    logits = rng.normal(0, 4, (9, 6))
    hard = (rng.random((9, 6)) < 0.3).astype(np.float64)
    lam = rng.uniform(0.5, 1.0, (9, 1))
    soft = lam * hard + (1 - lam) * hard[rng.permutation(9)]
    for y in (hard, soft):
        got = T.asymmetric_loss(torch.tensor(logits), torch.tensor(y), gamma_neg=gamma_neg)
        assert float(got) == pytest.approx(train_ref.asymmetric_loss_f64(logits, y, gamma_neg=gamma_neg), rel=1e-10)
        got32 = T.asymmetric_loss(torch.tensor(logits, dtype=torch.float32), torch.tensor(y, dtype=torch.float32), gamma_neg=gamma_neg)
        assert float(got32) == pytest.approx(train_ref.asymmetric_loss_f64(logits, y, gamma_neg=gamma_neg), rel=1e-4)
    # a confident right answer costs nothing, a confident wrong one much
    zero = T.asymmetric_loss(torch.tensor([[30.0, -30.0]]), torch.tensor([[1.0, 0.0]]), gamma_neg=gamma_neg)
    wrong = T.asymmetric_loss(torch.tensor([[-30.0, 30.0]]), torch.tensor([[1.0, 0.0]]), gamma_neg=gamma_neg)
    assert float(zero) == pytest.approx(0.0, abs=1e-9) and float(wrong) > 4.0


def test_mixed_cross_entropy_and_schedule():
    import torch
    import torch.nn.functional as F
    torch.manual_seed(0)
    logits, y, yp = torch.randn(6, 3), torch.tensor([0, 1, 2, 0, 1, 2]), torch.tensor([1, 1, 0, 2, 0, 2])
    assert float(T.mixed_cross_entropy(logits, y, yp, torch.ones(6))) == pytest.approx(float(F.cross_entropy(logits, y)))
    assert float(T.mixed_cross_entropy(logits, y, yp, torch.zeros(6))) == pytest.approx(float(F.cross_entropy(logits, yp)))
    lrs = [T.one_cycle(s, 100, 1e-3, 5.0, 0.3) for s in range(100)]
    assert lrs[0] == pytest.approx(2e-4) and max(lrs) == pytest.approx(1e-3) and int(np.argmax(lrs)) == 30 and lrs[-1] < 1e-5
    lrs = [T.one_cycle(s, 100, 1e-3, 25.0, 0.99) for s in range(100)]
    assert int(np.argmax(lrs)) == 99 and lrs[0] == pytest.approx(4e-5)


# ---- command line --------------------------------------------------------------------------------------------------

def test_every_reference_flag_parses():
    a = cli.parse_args(["train", "in", "out", "-R", "3", "-x", "-v", "-n", "4", "-t", "labels.csv", "-S", "-d", "0.6", "-V", "a,b",
                        "-f", "0.3", "-c", "fiannaca2018", "-m", "old.pt", "-b", "32", "-B", "2", "-C", "-r", "0.01", "-e", "7",
                        "-z", "2", "-w", "-i", "2", "-X", "CutMix", "-s", "-p", "0.5", "-l", "0.1", "-g", "-M",
                        "--input-size", "96"])
    want = dict(command="train", input="in", outdir="out", seed=3, overwrite=True, verbose=True, num_workers=4,
                label_table_path="labels.csv", single_label=True, threshold=0.6, validation_set="a,b",
                validation_set_fraction=0.3, architecture="fiannaca2018", pretrained_model="old.pt", max_batch_size=32,
                min_batch_size=2, cpu=True, base_learning_rate=0.01, epochs=7, freeze_epochs=2, random_weights=True,
                negative_downweighting=2.0, mix_augmentation="CutMix", label_smoothing=True, p_lighting=0.5, max_lighting=0.1,
                no_logging=True, no_metrics=True, input_size=96)
    assert vars(a) == want
    d = cli.parse_args(["train", "in", "out"])
    assert (d.threshold, d.validation_set_fraction, d.base_learning_rate, d.epochs, d.freeze_epochs) == (0.7, 0.2, 5e-3, 30, 0)
    assert (d.max_batch_size, d.min_batch_size, d.negative_downweighting, d.mix_augmentation) == (64, 1, 4, "MixUp")
    assert (d.p_lighting, d.max_lighting, d.num_workers, d.input_size) == (0.75, 0.25, 0, 224)
    assert d.architecture.startswith("hf-hub:")


def test_refusals(tmp_path, monkeypatch):
    (tmp_path / "in").mkdir()
    base = ["train", str(tmp_path / "in"), str(tmp_path / "out")]
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(_capi.VkError, match="no CPU fallback"):
        cli.main(base + ["-c", "arias2022", "-C"])
    for arch in ([], ["-c", "resnet50"], ["-c", "hf-hub:timm/vit_base_patch16_224.augreg"]):
        with pytest.raises(ValueError, match="timm or hub model.*arias2022, fiannaca2018, vit_l32, pkg.module:factory"):
            cli.main(base + arch)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(Exception, match="train runs on one GPU"):
        cli.main(base + ["-c", "arias2022"])
    monkeypatch.delenv("WORLD_SIZE")
    (tmp_path / "out").mkdir()
    with pytest.raises(Exception, match="Output directory exists"):
        cli.main(base + ["-c", "arias2022"])
    assert not list((tmp_path / "out").iterdir())


# ---- architectures and export --------------------------------------------------------------------------------------

def tiny_factory(n_classes):
    import torch
    return torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(4), torch.nn.Flatten(), torch.nn.Linear(48, n_classes))


@pytest.mark.parametrize("arch", ("arias2022", "fiannaca2018", "vit_l32", "test_train_rules:tiny_factory"))
def test_architectures_export_and_reload(arch, tmp_path):
    """Built, exported and read back by query.load_model on the CPU: equal logits at batch sizes 1 and 5 (the export
    itself probes 1 and 3).  vit_l32 is built here with a small width and depth -- the same code at a size a CPU test
    can afford; its default is ViT-L/32."""
    import torch
    from varkoder_amd import query
    torch.manual_seed(0)
    model, size = T.build_model(arch, 4, 32, 64, vit_kwargs=dict(dim=64, depth=2, heads=4, mlp=128))
    assert size == (32 if arch in T.NATIVE_SIZE_ARCHS else 64)
    assert T.last_linear(model).out_features == 4
    kind = T.export_model(model, tmp_path / "m.pt", size)
    assert kind in ("script", "trace")                 # does not depend on this package's classes
    loaded = query.load_model(tmp_path / "m.pt").eval()
    assert isinstance(loaded, torch.jit.ScriptModule)
    model.eval()
    for b in (1, 5):
        x = torch.randn(b, 3, size, size)
        with torch.no_grad():
            want, got = model(x), loaded(x)
        assert got.shape == (b, 4) and torch.allclose(got, want, rtol=1e-4, atol=1e-5)
    # -m: what matches by name and shape is copied in
    other, _ = T.build_model(arch, 7, 32, 64, vit_kwargs=dict(dim=64, depth=2, heads=4, mlp=128))
    n = T.load_matching_weights(other, tmp_path / "m.pt")
    sd, ref = other.state_dict(), model.state_dict()
    same = [k for k in sd if sd[k].shape == ref[k].shape]
    assert n == len(same) == len(sd) - 2               # all but the head's weight and bias
    assert all(torch.equal(sd[k], ref[k]) for k in same)
