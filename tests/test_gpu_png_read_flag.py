"""`--gpu-png-read` against the same run without it, on tiny inputs: pngread.read_images against PIL's route on a folder
that mixes eligible files, split IDATs, files PIL must take and a damaged one; train's image set; query --images'
predictions.csv; train's exported files."""
import os
import shutil
import warnings

import numpy as np
import pytest

import png_cases as P
import unpng_cases as U

pytestmark = pytest.mark.gpu


def pil_route(paths, device):
    """What both commands do without the flag."""
    import torch
    from PIL import Image
    return torch.from_numpy(np.stack([np.array(Image.open(p)) for p in paths])).to(device)


def outcome(fn):
    try:
        return "ok", fn()
    except Exception as e:   # noqa: BLE001 -- the type is what is compared
        return type(e), None


@pytest.fixture(scope="module")
def eng(engines):
    return engines(7)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Side 65: PIL's own files and forced filters with split IDATs (eligible), and two palette files (PIL's to decode:
    bytes of the same shape), one in the middle and one at the end."""
    from PIL import Image
    from varkoder_amd import pngread as R
    d = tmp_path_factory.mktemp("png_read")
    paths = []
    for i, (name, data, arr) in enumerate(U.by_side()[65][:12]):
        p = d / f"f{i:02d}.png"
        p.write_bytes(data)
        paths.append(p)
    assert any(len(R.png_parts(p.read_bytes()).spans) > 1 for p in paths) and all(R.eligible(R.png_parts(p.read_bytes())) for p in paths)
    grey = U.images()["s65_levels7"]
    for name in ("palette_a.png", "palette_b.png"):
        Image.fromarray(grey if name.endswith("a.png") else grey.T.copy()).convert("P").save(d / name, format="PNG")
        assert not R.eligible(R.png_parts((d / name).read_bytes()))
    return d, paths[:5] + [d / "palette_a.png"] + paths[5:] + [d / "palette_b.png"]


def damaged_file(arr, how):
    stream = bytearray(U.deflated(U.filtered(arr, 4), "level9"))
    if how == "adler":
        stream[-1] ^= 1
    elif how == "cut":
        stream = stream[:len(stream) // 2]
    return U.write(arr.shape[0], bytes(stream))


def test_read_images_equals_the_pil_route_on_a_mixed_folder(eng, folder):
    import torch
    from varkoder_amd import pngread as R
    d, paths = folder
    got = R.read_images(eng, paths)
    want = pil_route(paths, eng.device)
    assert got.dtype == want.dtype == torch.uint8 and got.device == want.device and torch.equal(got, want)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:
        assert torch.equal(R.read_images(eng, paths, pool=pool), want)
    # a file PIL must take among them: 16-bit is not bytes, so the whole set goes PIL's way; an RGB one has another shape
    from PIL import Image
    Image.fromarray(np.zeros((65, 65), dtype=np.uint16)).save(d / "wide.png")
    a, b = outcome(lambda: R.read_images(eng, paths + [d / "wide.png"])), outcome(lambda: pil_route(paths + [d / "wide.png"], eng.device))
    assert a[0] == b[0] and (a[0] != "ok" or (a[1].dtype == b[1].dtype and torch.equal(a[1], b[1])))
    Image.fromarray(np.zeros((65, 65, 3), dtype=np.uint8)).save(d / "rgb.png")
    with pytest.raises(Exception, match="^Images of different sizes in one query are not supported.$"):
        R.read_images(eng, paths + [d / "rgb.png"], mixed="Images of different sizes in one query are not supported.")
    only = R.read_images(eng, [d / "rgb.png", d / "rgb.png"])
    assert torch.equal(only, pil_route([d / "rgb.png"] * 2, eng.device))
    os.remove(d / "wide.png")
    os.remove(d / "rgb.png")


@pytest.mark.parametrize("how", ["adler", "cut"])
def test_the_two_routes_agree_on_a_damaged_file(eng, folder, tmp_path, how):
    import torch
    from varkoder_amd import pngread as R
    d, paths = folder
    bad = tmp_path / "bad.png"
    bad.write_bytes(damaged_file(U.images()["s65_uniform"], how))
    assert R.eligible(R.png_parts(bad.read_bytes()))
    mixed = paths[:3] + [bad] + paths[3:6]
    a, b = outcome(lambda: R.read_images(eng, mixed)), outcome(lambda: pil_route(mixed, eng.device))
    print(how, a[0], b[0])
    assert a[0] == b[0]
    if a[0] == "ok":
        assert torch.equal(a[1], b[1])


def test_mixed_sizes_raise_todays_message(eng, folder, tmp_path):
    from varkoder_amd import pngread as R, train as T
    d, paths = folder
    other = tmp_path / "s64.png"
    other.write_bytes(U.files()["s64_levels7/pil"][0])
    for fn in (lambda: T.image_set(paths[:2] + [other]), lambda: T.image_set(paths[:2] + [other], eng)):
        with pytest.raises(Exception, match="^Images of different sizes in one training run are not supported.$"):
            fn()
    with pytest.raises(Exception, match="^Images of different sizes in one query are not supported.$"):
        R.read_images(eng, paths[:2] + [other], mixed="Images of different sizes in one query are not supported.")


def test_trains_image_set_is_the_same_with_and_without_the_engine(eng, folder):
    import torch
    from varkoder_amd import train as T
    d, paths = folder
    host, dev = T.image_set(paths), T.image_set(paths, eng)
    assert host.dtype == dev.dtype == torch.uint8 and host.device.type == "cpu" and dev.device == eng.device
    assert tuple(host.shape) == tuple(dev.shape) == (len(paths), 65, 65) and torch.equal(host.to(eng.device), dev)


def _tiny_model(path, classes):   # (the seeded model of tests/test_query.py)
    import torch

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pool = torch.nn.AdaptiveAvgPool2d(6)
            self.fc = torch.nn.Linear(3 * 36, classes)

        def forward(self, x):
            return self.fc(self.pool(x).flatten(1))
    torch.manual_seed(3)
    m = Tiny()
    with torch.no_grad():
        m.fc.weight.mul_(40.0)
    torch.jit.script(m).save(str(path))


def test_query_images_writes_the_same_predictions(tmp_path):
    import glob
    from varkoder_amd import cli
    from varkoder_amd.image import write_png
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    indir = tmp_path / "imgs" / "sub"
    indir.mkdir(parents=True)
    for p in sorted(glob.glob(os.path.join(golden, "docs_*+cgr+k7.png"))):
        shutil.copyfile(p, indir / os.path.basename(p)[len("docs_"):])
    arr = P.cases()["s128_levels7"]
    write_png(arr, indir / "mine@00010000K+cgr+k7.png", ["kingdom:Fungi"], 0.02, 0.01, "cgr")
    (indir / "split@00020000K+cgr+k7.png").write_bytes(U.forced(arr.T.copy(), "mix", "level9", "seven"))   # (no text chunks)
    vocab = ["kingdom:Animalia", "kingdom:Bacteria", "kingdom:Fungi", "x", "y"]
    (tmp_path / "vocab.txt").write_text("\n".join(vocab) + "\n")
    _tiny_model(tmp_path / "m.pt", len(vocab))
    common = ["query", "--images", "-l", str(tmp_path / "m.pt"), "--vocab", str(tmp_path / "vocab.txt"), "-P", "-d", "0.6",
              str(tmp_path / "imgs")]
    cli.main(common + [str(tmp_path / "A")])
    cli.main(common + [str(tmp_path / "B"), "--gpu-png-read"])
    a, b = (tmp_path / "A" / "predictions.csv").read_text(), (tmp_path / "B" / "predictions.csv").read_text()
    assert a == b and a.count("\n") == 6 and "kingdom:Fungi" in a


def test_query_without_images_refuses_the_flag(capsys):
    from varkoder_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["query", "in", "out", "-l", "m", "--vocab", "v", "--gpu-png-read"])
    assert "--gpu-png-read: only with -I/--images" in capsys.readouterr().err


def test_train_on_a_dozen_images_writes_the_same_labels(tmp_path):
    from varkoder_amd import cli, train as T
    from varkoder_amd.config import QUAL_THRESH
    from varkoder_amd.image import write_png
    rng = np.random.default_rng(7)
    root = tmp_path / "images"
    root.mkdir()
    for s in range(6):
        cls = "A" if s % 2 == 0 else "B"
        for bp in (500, 1000):
            img = rng.integers(0, 96, (32, 32))
            img[:, :16] += 128 if cls == "A" else 0
            img[:, 16:] += 128 if cls == "B" else 0
            write_png(img.astype(np.uint8), root / f"s{s:02d}@{bp:08d}K+cgr+k5.png", [f"genus:{cls}", "family:F"], 0.001,
                      QUAL_THRESH, "cgr")
    outs = []
    for flags in ([], ["--gpu-png-read"]):
        out = tmp_path / ("with" if flags else "without")
        args = cli.parse_args(["train", str(root), str(out), "-c", "arias2022", "-R", "1", "-g", "-S", "-X", "None", "-p", "0",
                               "-e", "1", "-B", "4"] + flags)
        with warnings.catch_warnings():   # (the label-mode warnings of check_label_types)
            warnings.simplefilter("ignore")
            history = T.run_train(args)
        assert len(history) == 1 and (out / "trained_model.pt").is_file() and (out / "labels.txt").is_file()
        outs.append(((out / "labels.txt").read_text(), (out / "input_data.csv").read_text(), history))
    assert outs[0][0] == outs[1][0] and len(outs[0][0].split()) == 2
    assert outs[0][1] == outs[1][1]
