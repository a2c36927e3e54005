"""`varKoder train` (commands/train.py, cli.py:168-323): fit a classifier on varKode / rfCGR images and write the two
files `query -l MODEL --vocab LABELS` takes.

The training set is uploaded once as uint8 [N, side, side] and stays in HBM; every step one HIP launch
(vk_train_batch_device, csrc/vk_train.h) turns a list of indices into the model's input batch: gather, PIL-exact BOX
squish, lighting, MixUp / CutMix, normalise, three channels.  The reference decodes every PNG again each epoch in
DataLoader workers and runs these as a chain of fastai transforms; fastai, timm and their pretrained weights are not
assumed here, so the batch rule, the schedule and the architectures are this project's own statement of them
("train", lists the rule and the known differences).  Model and optimiser are plain PyTorch; there is
no CPU path.
"""
import ctypes as C
import importlib
import math
import os
import warnings
from pathlib import Path

import numpy as np

from . import _capi
from .config import LABELS_SEP
from .image import eprint

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2
MODES = {"None": MODE_NONE, "MixUp": MODE_MIXUP, "CutMix": MODE_CUTMIX}
ARCHITECTURES = ("arias2022", "fiannaca2018", "vit_l32", "pkg.module:factory")
NATIVE_SIZE_ARCHS = ("arias2022", "fiannaca2018")
LOW_QUALITY_LABEL = "low_quality:True"
MEAN = STD = 0.5   # what query.preprocess feeds a model by default: a trained model sees the same


# ---- the input table (collect_images, commands/train.py:396-439) ---------------------------------------------------

def collect_images(src, label_table=None, verbose=False):
    """One row per *.png under src (recursively, in sorted order): sample, bp, img_kmer_mapping, img_kmer_size and path
    from the file name, labels and possible_low_quality from the PNG's text chunks -- or, with a label table, labels
    from its `sample,labels` columns by inner join (samples it lacks are dropped and counted on stderr)."""
    import pandas as pd
    from PIL import Image
    from .convert import get_metadata_from_img_filename
    from .query import image_metadata
    eprint("Collecting image files for training...")
    rows = [get_metadata_from_img_filename(p) for p in sorted(Path(src).rglob("*.png"))]
    eprint(f"Found {len(rows)} image files")
    if not rows:
        raise Exception("No images found to train on. Please check your input.")
    df = pd.DataFrame(rows)
    if label_table:
        table = pd.read_csv(label_table, dtype=str).fillna("")[["sample", "labels"]]
        merged = df.merge(table, on="sample", how="inner")
        excluded = sorted(set(df["sample"]) - set(merged["sample"]))
        eprint(len(excluded), "samples excluded due to absence in provided label table.")
        if verbose:
            eprint("Samples excluded:\n", "\n".join(excluded))
        return merged
    labels, qual = [], []
    for p in df["path"]:
        with Image.open(p) as im:
            lab, q, _ = image_metadata(im.info)
        labels.append(lab if isinstance(lab, str) else "")
        qual.append(q)
    return df.assign(labels=labels, possible_low_quality=qual)


def sort_labels(text):
    return LABELS_SEP.join(sorted(text.split(LABELS_SEP)))


def validation_split(df, validation_set=None, fraction=0.2, seed=None):
    """df with its labels sorted within each row and an `is_valid` column (commands/train.py:441-485).  validation_set: a
    file whose first line is a comma list of samples, or such a list itself.  Otherwise a fraction of the distinct
    samples of every (sorted) label combination -- round(fraction * their number), drawn without replacement by
    numpy.random.default_rng(seed) from the sorted sample names, combinations in sorted order -- so a sample's images
    all stay on one side."""
    df = df.assign(labels=df["labels"].apply(sort_labels))
    if validation_set:
        eprint("Splitting validation set as defined by user.")
        try:
            with open(validation_set) as f:
                held = f.readline().strip().split(",")
        except OSError:
            held = str(validation_set).split(",")
    else:
        eprint("Splitting validation set randomly. Fraction of samples per label combination held as validation:",
               str(fraction))
        rng = np.random.default_rng(seed)
        pairs = df[["sample", "labels"]].drop_duplicates()
        held = []
        for _, group in sorted(pairs.groupby("labels"), key=lambda kv: kv[0]):
            names = sorted(group["sample"])
            take = round(fraction * len(names))
            held.extend(names[i] for i in sorted(rng.choice(len(names), size=take, replace=False)))
    return df.assign(is_valid=df["sample"].isin(set(held)))


def check_label_types(df, single_label):
    """The reference's two warnings about a label mode that does not fit the labels (commands/train.py:487-507)."""
    several = bool(df["labels"].str.contains(LABELS_SEP).any())
    if single_label:
        eprint("Single label model requested.")
        if several:
            warnings.warn("Some samples contain more than one label. These will be concatenated. "
                          "Maybe you want a multilabel model instead?", stacklevel=2)
    else:
        eprint("Multilabel model requested.")
        if not several:
            warnings.warn("No sample contains more than one label. Maybe you want a single label model instead?",
                          stacklevel=2)


def vocabulary(df, single_label):
    """Output units in order: the sorted distinct labels, or (-S) the sorted distinct joined label strings."""
    if single_label:
        return sorted(set(df["labels"]))
    return sorted({x for text in df["labels"] for x in text.split(LABELS_SEP)})


def targets(df, vocab, single_label):
    """int64 [N] class indices (-S) or float32 [N, len(vocab)] multi-hot rows."""
    where = {v: i for i, v in enumerate(vocab)}
    if single_label:
        return np.array([where[text] for text in df["labels"]], dtype=np.int64)
    y = np.zeros((len(df), len(vocab)), dtype=np.float32)
    for r, text in enumerate(df["labels"]):
        for x in text.split(LABELS_SEP):
            y[r, where[x]] = 1.0
    return y


def batch_size(n_train, min_bs=1, max_bs=64):
    """A power of two that splits the training set into about ten batches, clamped (commands/train.py:226-228)."""
    bs = 2 ** round(math.log2(n_train / 10))
    return int(max(min(bs, max_bs), min_bs))


# ---- augmentation parameters ---------------------------------------------------------------------------------------

def cutmix_rect(t, cx, cy, out):
    """(x1, y1, x2, y2, lam) of CutMix for one draw t in [0, 1] and a centre: a square of round(out * sqrt(1 - t)) per
    side around (cx, cy), clipped to the image; lam = 1 - area / out^2 of what is left."""
    w = int(round(out * math.sqrt(max(0.0, 1.0 - t))))
    x1, y1 = cx - w // 2, cy - w // 2
    x2, y2 = x1 + w, y1 + w
    x1, y1, x2, y2 = (min(max(int(v), 0), out) for v in (x1, y1, x2, y2))
    return x1, y1, x2, y2, 1.0 - (x2 - x1) * (y2 - y1) / float(out * out)


def draw_batch_params(gen, B, out, mode, p_lighting, max_lighting):
    """One step's augmentation parameters as plain numpy arrays, drawn from the torch.Generator `gen` (CPU):
    {"partner": uint32 [B], "lam": float32 [B], "bshift": float32 [B], "cscale": float32 [B], "rect": (x1, y1, x2, y2)}.

    Brightness: with probability p per item b ~ U(0.5 (1 - l), 0.5 (1 + l)) and bshift = log(b / (1 - b)), else 0.
    Contrast: with an independent probability p, cscale = exp(U(log(1 - l), -log(1 - l))), else 1.  l = 0 or p = 0:
    every row neutral.  MixUp: lam = max(t, 1 - t), t ~ Beta(0.4, 0.4) per item; CutMix: one t ~ Beta(1, 1) per step
    and cutmix_rect around a uniform centre, its lam for every item; partner is a random permutation for both, and the
    identity with lam = 1 without a mix.  The same number of draws is made whatever p and l are."""
    import torch
    if not 0.0 <= max_lighting < 1.0:
        raise ValueError("max lighting must be in [0, 1)")
    l, p = float(max_lighting), float(p_lighting)
    u = torch.rand((4, B), generator=gen, dtype=torch.float64).numpy()
    bshift = np.zeros(B, dtype=np.float32)
    cscale = np.ones(B, dtype=np.float32)
    if l > 0.0 and p > 0.0:
        b = 0.5 * (1.0 - l) + u[1] * l
        bshift = np.where(u[0] < p, np.log(b / (1.0 - b)), 0.0).astype(np.float32)
        span = -math.log(1.0 - l)
        cscale = np.where(u[2] < p, np.exp((2.0 * u[3] - 1.0) * span), 1.0).astype(np.float32)
    partner = np.arange(B, dtype=np.uint32)
    lam = np.ones(B, dtype=np.float32)
    rect = (0, 0, 0, 0)

    def beta(a, n):
        g = torch._standard_gamma(torch.full((2, n), a, dtype=torch.float64), generator=gen).numpy()
        s = g[0] + g[1]
        return np.where(s > 0.0, g[0] / np.where(s > 0.0, s, 1.0), 0.5)
    if mode == MODE_MIXUP:
        t = beta(0.4, B)
        lam = np.clip(np.maximum(t, 1.0 - t), 0.0, 1.0).astype(np.float32)
        partner = torch.randperm(B, generator=gen).numpy().astype(np.uint32)
    elif mode == MODE_CUTMIX:
        t = float(beta(1.0, 1)[0])
        cx, cy = (int(v) for v in torch.randint(0, out, (2,), generator=gen))
        x1, y1, x2, y2, lm = cutmix_rect(t, cx, cy, out)
        rect = (x1, y1, x2, y2)
        lam = np.full(B, lm, dtype=np.float32)
        partner = torch.randperm(B, generator=gen).numpy().astype(np.uint32)
    elif mode != MODE_NONE:
        raise ValueError("mode is 0 (none), 1 (MixUp) or 2 (CutMix)")
    return {"partner": partner, "lam": lam, "bshift": bshift, "cscale": cscale, "rect": rect}


def train_batch(engine, images, idx, partner, lam, bshift, cscale, rect=(0, 0, 0, 0), mode=MODE_NONE, out_size=224,
                mean=MEAN, std=STD, out=None):
    """The model's input for one step (vk_train_batch_device): uint8 device tensor images [N, side, side] and host
    arrays of length B -> float32 device tensor [B, 3, out, out]."""
    import torch
    from .query import box_tables
    n, side, side2 = images.shape
    assert side == side2 and images.dtype == torch.uint8 and images.is_contiguous()
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    partner = np.ascontiguousarray(partner, dtype=np.uint32)
    lam, bshift, cscale = (np.ascontiguousarray(a, dtype=np.float32) for a in (lam, bshift, cscale))
    B = len(idx)
    if not (len(partner) == len(lam) == len(bshift) == len(cscale) == B):
        raise ValueError("one partner, lam, bshift and cscale per row of the batch")
    cache = engine.__dict__.setdefault("_box_tables", {})
    if (side, out_size) not in cache:
        cache[(side, out_size)] = box_tables(side, out_size)
    bounds, coef = cache[(side, out_size)]
    if out is None:
        out = torch.empty((B, 3, out_size, out_size), dtype=torch.float32, device=images.device)
    assert out.shape == (B, 3, out_size, out_size) and out.dtype == torch.float32 and out.is_contiguous()
    assert out.device == images.device
    x1, y1, x2, y2 = (int(v) for v in rect)
    if min(x1, y1, x2, y2) < 0:
        raise _capi.VkError(_capi.VK_EINVAL, "vk_train_batch_device: a rectangle outside the image")
    u32p = C.POINTER(C.c_uint32)
    st = engine.L.vk_train_batch_device(
        engine.ctx, C.c_void_p(images.data_ptr()), n, side, out_size, C.c_void_p(bounds.ctypes.data),
        C.c_void_p(coef.ctypes.data), coef.shape[1], C.c_float(mean), C.c_float(std), B, idx.ctypes.data_as(u32p),
        partner.ctypes.data_as(u32p), C.c_void_p(lam.ctypes.data), C.c_void_p(bshift.ctypes.data),
        C.c_void_p(cscale.ctypes.data), x1, y1, x2, y2, int(mode), C.c_void_p(out.data_ptr()))
    _capi.check(engine.ctx, st, "vk_train_batch_device")
    return out


def plain_batch(engine, images, out_size):
    """Validation input, no augmentation: query.preprocess -- or, for a native-size image too large for its LDS
    intermediate (512 x 512), the batch kernel with every row neutral, which writes the same bits without one."""
    from .query import preprocess
    n, side = images.shape[0], images.shape[1]
    if side == out_size and side * out_size > 160 * 1024 - 1024:
        return train_batch(engine, images, np.arange(n), np.arange(n), np.ones(n), np.zeros(n), np.ones(n),
                           out_size=out_size)
    return preprocess(engine, images, out_size=out_size, mean=MEAN, std=STD)


# ---- models --------------------------------------------------------------------------------------------------------

def is_factory(architecture):
    """`pkg.module:factory`, as opposed to a hub name such as `hf-hub:owner/model`."""
    return ":" in architecture and not architecture.startswith("hf-hub:") and "/" not in architecture


def refusal_of(architecture):
    return (f"architecture {architecture!r} is a timm or hub model, and timm and its pretrained weights are not "
            f"available to this build: choose one of {', '.join(ARCHITECTURES)}")


def build_model(architecture, n_classes, side, input_size=None, vit_kwargs=None):
    """(model, side of its input).  arias2022 and fiannaca2018 (the layer lists of commands/train.py:51-123, with the
    sizes the reference's lazy layers would take written out) read one channel at the images' own size; vit_l32 is
    query.vit() with an n_classes head at input_size (224); `pkg.module:factory` calls factory(n_classes).  Weights
    are random.  A timm or hub name is refused: timm is not assumed here."""
    import torch
    from torch import nn

    class OneChannel(nn.Module):
        """[B, 3, H, W] -> [B, H * W]: the first channel, flattened."""

        def forward(self, x):
            return x[:, 0].flatten(1)

    class AsSequence(nn.Module):
        def forward(self, x):
            return x.unsqueeze(1)

    if architecture == "arias2022":
        body = nn.Sequential(OneChannel(), nn.Linear(side * side, 512), nn.ReLU(), nn.Dropout(0.5), nn.Linear(512, 64),
                             nn.ReLU(), nn.Dropout(0.5))
        return nn.Sequential(body, nn.Linear(64, n_classes)), side
    if architecture == "fiannaca2018":
        length = ((side * side - 4) // 2 - 4) // 2
        if length < 1:
            raise ValueError("fiannaca2018: images too small")
        body = nn.Sequential(OneChannel(), AsSequence(), nn.Conv1d(1, 5, kernel_size=5), nn.ReLU(), nn.MaxPool1d(2),
                             nn.Conv1d(5, 10, kernel_size=5), nn.ReLU(), nn.MaxPool1d(2), nn.Flatten(),
                             nn.Linear(10 * length, 500), nn.ReLU())
        return nn.Sequential(body, nn.Linear(500, n_classes)), side
    if architecture == "vit_l32":
        from .query import vit
        size = input_size or 224
        return vit(img_size=size, num_classes=n_classes, **(vit_kwargs or {})), size
    if is_factory(architecture):
        module, _, name = architecture.partition(":")
        model = getattr(importlib.import_module(module), name)(n_classes)
        if not isinstance(model, torch.nn.Module):
            raise TypeError(f"{architecture}: the factory must return a torch.nn.Module")
        return model, input_size or 224
    raise ValueError(refusal_of(architecture))


def last_linear(model):
    from torch import nn
    found = None
    for m in model.modules():
        if isinstance(m, nn.Linear):
            found = m
    if found is None:
        raise ValueError("the model has no nn.Linear to train during the frozen epochs")
    return found


def load_matching_weights(model, path):
    """-m: the entries of the file's state dict that the model has under the same name and shape are copied in
    (commands/train.py:338-345); returns how many."""
    from .query import load_model
    have = model.state_dict()
    new = {k: v for k, v in load_model(path).state_dict().items() if k in have and have[k].shape == v.shape}
    model.load_state_dict(new, strict=False)
    return len(new)


def export_model(model, path, input_size):
    """trained_model.pt on the CPU in eval mode: a TorchScript archive (scripted; traced if the model does not script),
    kept only if it reproduces the eager logits at batch sizes 1 and 3 -- else the pickled module, which query.load_model
    reads as well but which needs the model's classes importable.  Returns "script", "trace" or "pickle"."""
    import torch
    model = model.float().cpu().eval()
    gen = torch.Generator().manual_seed(0)
    probes = [torch.randn((b, 3, input_size, input_size), generator=gen) for b in (1, 3)]
    with torch.no_grad():
        want = [model(x) for x in probes]

    def faithful(m):
        with torch.no_grad():
            return all(torch.allclose(m(x), w, rtol=1e-4, atol=1e-5) for x, w in zip(probes, want))
    for kind, make in (("script", lambda: torch.jit.script(model)),
                       ("trace", lambda: torch.jit.trace(model, probes[1], check_trace=False))):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                scripted = make()
                ok = faithful(scripted)
        except Exception:   # noqa: BLE001 -- a model TorchScript cannot take: the next form
            continue
        if ok:
            scripted.save(str(path))
            return kind
    torch.save(model, str(path))
    return "pickle"


# ---- losses --------------------------------------------------------------------------------------------------------

def asymmetric_loss(logits, y, gamma_neg=4.0, gamma_pos=0.0, clip=0.1, eps=1e-2):
    """The asymmetric multilabel loss (Ridnik et al. 2021, arXiv:2009.14119) on hard or soft targets y in [0, 1], summed
    over items and labels.  With p = sigmoid(logits) and m = min(1 - p + clip, 1):

        L = - sum( w * ( y * log(max(p, eps)) + (1 - y) * log(max(m, eps)) ) )
        w = (1 - (p * y + m * (1 - y))) ** (gamma_pos * y + gamma_neg * (1 - y))        (w = 1 when both gammas are 0)

    `train` uses gamma_pos = 0, gamma_neg = -i, eps = 1e-2, clip = 0.1, and y = lam * y_i + (1 - lam) * y_partner."""
    import torch
    p = torch.sigmoid(logits if logits.dtype == torch.float64 else logits.float())   # (fp16 logits under autocast)
    m = (1.0 - p + clip).clamp(max=1.0) if clip and clip > 0 else 1.0 - p
    loss = y * torch.log(p.clamp(min=eps)) + (1.0 - y) * torch.log(m.clamp(min=eps))
    if gamma_neg > 0 or gamma_pos > 0:
        loss = loss * torch.pow(1.0 - (p * y + m * (1.0 - y)), gamma_pos * y + gamma_neg * (1.0 - y))
    return -loss.sum()


def mixed_cross_entropy(logits, y, y_partner, lam, smoothing=0.0):
    """Per-item cross entropy against both targets, blended by lam, averaged over the batch."""
    import torch.nn.functional as F
    a = F.cross_entropy(logits.float(), y, reduction="none", label_smoothing=smoothing)
    b = F.cross_entropy(logits.float(), y_partner, reduction="none", label_smoothing=smoothing)
    return (lam * a + (1.0 - lam) * b).mean()


def one_cycle(step, total, peak, start_div, pct_peak, final_div=1e5):
    """Learning rate of step `step` of `total`: cosine from peak / start_div up to peak at pct_peak of the phase, then
    cosine down to peak / final_div."""
    t = step / max(total, 1)
    lo, a = (peak / start_div, t / pct_peak) if t < pct_peak else (peak / final_div, (1.0 - t) / (1.0 - pct_peak))
    return lo + (peak - lo) * 0.5 * (1.0 - math.cos(math.pi * min(max(a, 0.0), 1.0)))


def micro_precision_recall(probs, y, threshold, keep):
    """Micro-averaged precision and recall at a threshold over the label columns `keep`."""
    pred, true = probs[:, keep] >= threshold, y[:, keep] > 0.5
    tp = float((pred & true).sum())
    return (tp / float(pred.sum()) if pred.any() else 0.0), (tp / float(true.sum()) if true.any() else 0.0)


# ---- the command ---------------------------------------------------------------------------------------------------

def refuse_early(args):
    """What can be refused before anything is read or the GPU is touched."""
    from .shard import world_info
    if args.cpu:
        raise _capi.VkError(_capi.VK_EHIP, "-C/--cpu: training on the CPU is not available: the HIP path cannot run "
                                           "(no CPU fallback)")
    if world_info()[1] > 1:
        raise Exception("train runs on one GPU: start it without a launcher (WORLD_SIZE > 1 is refused; the "
                        "reference's DataParallel is not rebuilt here)")
    if args.architecture not in NATIVE_SIZE_ARCHS + ("vit_l32",) and not is_factory(args.architecture):
        raise ValueError(refusal_of(args.architecture))
    if not args.overwrite and Path(args.outdir).exists():
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")


def image_set(paths, eng=None):
    """The training set's images, uint8 [n, side, side]: decoded by PIL on the host (a CPU tensor: the caller moves it),
    or with an engine by pngread.read_images where they will stay (a device tensor; --gpu-png-read).  Both routes give
    the same bytes and refuse the same sets with the same message."""
    import torch
    from PIL import Image
    message = "Images of different sizes in one training run are not supported."
    if eng is not None:
        from .pngread import read_images
        images = read_images(eng, paths, mixed=message)
        if images.dim() != 3 or images.shape[1] != images.shape[2]:
            raise Exception(message)
        return images.to(torch.uint8)
    arrays = [np.array(Image.open(p)) for p in paths]
    if len({a.shape for a in arrays}) > 1 or arrays[0].ndim != 2 or arrays[0].shape[0] != arrays[0].shape[1]:
        raise Exception(message)
    return torch.from_numpy(np.stack(arrays).astype(np.uint8))


def run_train(args):
    """The `train` sub-command; returns the per-epoch history (a list of dicts: phase, epoch, train_loss and, unless -M,
    valid_loss with accuracy or precision / recall)."""
    import torch
    from .engine import ImageEngine
    from .shard import world_info
    refuse_early(args)
    eprint("Starting train command.")
    df = collect_images(args.input, args.label_table_path, args.verbose)
    df = validation_split(df, args.validation_set, args.validation_set_fraction, args.seed)
    check_label_types(df, args.single_label)
    single = bool(args.single_label)
    mode = MODES[args.mix_augmentation]
    vocab = vocabulary(df, single)
    y_all = targets(df, vocab, single)
    train_rows = np.flatnonzero(~df["is_valid"].to_numpy())
    valid_rows = np.flatnonzero(df["is_valid"].to_numpy())
    if len(train_rows) == 0:
        raise Exception("No training images left after the validation split.")
    B = batch_size(len(train_rows), args.min_batch_size, args.max_batch_size)
    if B > len(train_rows):
        raise Exception(f"Batch size {B} exceeds the {len(train_rows)} training images (the last short batch is dropped).")
    device = world_info()[2]
    k = int(df["img_kmer_size"].iloc[0])
    # --gpu-png-read: the engine decodes the files, so it exists before the model does
    eng = ImageEngine(k=k, mapping="cgr", device=device) if getattr(args, "gpu_png_read", False) else None
    try:
        images = image_set(df["path"], eng)
        side = int(images.shape[1])

        eprint("Setting up neural network model for training.")
        seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(4), "little")
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        model, out_size = build_model(args.architecture, len(vocab), side, getattr(args, "input_size", None))
        if args.pretrained_model:
            eprint("Loading pretrained model from file:", str(args.pretrained_model))
            eprint(load_matching_weights(model, args.pretrained_model), "tensors taken from it.")
        else:
            eprint("Starting model with random weights.")
        eprint("Model architecture:", args.architecture)

        if eng is None:
            eng = ImageEngine(k=k, mapping="cgr", device=device)
        images = images.to(eng.device)   # resident from here on
        y_dev = torch.from_numpy(y_all).to(eng.device)
        model = model.to(eng.device)
        keep = [i for i, v in enumerate(vocab) if v != LOW_QUALITY_LABEL]
        scaler = torch.amp.GradScaler("cuda")
        smoothing = 0.1 if args.label_smoothing else 0.0
        history = []

        def loss_of(logits, rows, params):
            if not single:
                lam = torch.from_numpy(params["lam"]).to(eng.device)[:, None] if mode else 1.0
                soft = y_dev[rows] if not mode else lam * y_dev[rows] + (1.0 - lam) * y_dev[rows[params["partner"].astype(np.int64)]]
                return asymmetric_loss(logits, soft, gamma_neg=args.negative_downweighting)
            if not mode:
                return torch.nn.functional.cross_entropy(logits.float(), y_dev[rows])
            lam = torch.from_numpy(params["lam"]).to(eng.device)
            return mixed_cross_entropy(logits, y_dev[rows], y_dev[rows[params["partner"].astype(np.int64)]], lam, smoothing)

        def validate():
            model.eval()
            total, probs = 0.0, []
            with torch.no_grad():
                for s in range(0, len(valid_rows), B):
                    rows = valid_rows[s:s + B]
                    x = plain_batch(eng, images[torch.from_numpy(rows).to(eng.device)].contiguous(), out_size)
                    with torch.autocast("cuda", dtype=torch.float16):
                        logits = model(x)
                    if single:
                        total += float(torch.nn.functional.cross_entropy(logits.float(), y_dev[rows], reduction="sum"))
                        probs.append(torch.softmax(logits.float(), dim=1).cpu().numpy())
                    else:
                        total += float(asymmetric_loss(logits, y_dev[rows], gamma_neg=args.negative_downweighting))
                        probs.append(torch.sigmoid(logits.float()).cpu().numpy())
            probs = np.concatenate(probs)
            got = {"valid_loss": total / len(valid_rows)}
            if single:
                got["accuracy"] = float((probs.argmax(axis=1) == y_all[valid_rows]).mean())
            else:
                got["precision"], got["recall"] = micro_precision_recall(probs, y_all[valid_rows], args.threshold, keep)
            return got

        def phase(name, epochs, params, peak, start_div, pct_peak):
            if epochs <= 0:
                return
            opt = torch.optim.AdamW(params, lr=peak, betas=(0.9, 0.99), eps=1e-5, weight_decay=0.01)
            steps_per_epoch = len(train_rows) // B
            total, step = epochs * steps_per_epoch, 0
            for epoch in range(epochs):
                model.train()
                order = train_rows[torch.randperm(len(train_rows), generator=gen).numpy()]
                seen, running = 0, 0.0
                for s in range(steps_per_epoch):
                    rows = order[s * B:(s + 1) * B]
                    aug = draw_batch_params(gen, B, out_size, mode, args.p_lighting, args.max_lighting)
                    x = train_batch(eng, images, rows, aug["partner"], aug["lam"], aug["bshift"], aug["cscale"], aug["rect"],
                                    mode, out_size)
                    for g in opt.param_groups:
                        g["lr"] = one_cycle(step, total, peak, start_div, pct_peak)
                    with torch.autocast("cuda", dtype=torch.float16):
                        logits = model(x)
                    loss = loss_of(logits, rows, aug)
                    opt.zero_grad(set_to_none=True)
                    scaler.scale(loss).backward()
                    scaler.step(opt)
                    scaler.update()
                    step += 1
                    running += float(loss.detach())
                    seen += 1
                row = {"phase": name, "epoch": epoch, "train_loss": running / max(seen, 1)}
                if not args.no_metrics and len(valid_rows):
                    row.update(validate())
                history.append(row)
                if not args.no_logging:
                    eprint("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()))

        eprint("Start training for", args.freeze_epochs, "epochs with frozen model body weights followed by", args.epochs,
               "epochs with unfrozen weights and learning rate of", args.base_learning_rate)
        if args.freeze_epochs > 0:
            head = last_linear(model)
            for p in model.parameters():
                p.requires_grad_(False)
            for p in head.parameters():
                p.requires_grad_(True)
            phase("frozen", args.freeze_epochs, list(head.parameters()), args.base_learning_rate, 25.0, 0.99)
            for p in model.parameters():
                p.requires_grad_(True)
        phase("unfrozen", args.epochs, list(model.parameters()), args.base_learning_rate / 2.0, 5.0, 0.3)
        torch.cuda.synchronize(eng.device)
    finally:
        if eng is not None:
            eng.close()

    outdir = Path(args.outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    kind = export_model(model, outdir / "trained_model.pt", out_size)
    with open(outdir / "labels.txt", "w") as f:
        f.write("\n".join(vocab) + "\n")
    df.assign(path=df["path"].astype(str)).to_csv(outdir / "input_data.csv", index=False)
    eprint("Model (" + kind + "), labels, and data table saved to directory", str(outdir))
    return history
