"""The batch rule of `train` ("train"; vk_train_batch_device) restated on the host: once in numpy
float64, the reference the kernel is held to, and once in float32 torch-CPU ops, whose own distance from the float64
result sizes the tolerance.  No GPU, nothing imported from the kernel's side but the BOX coefficient tables."""
import numpy as np

from varkoder_amd import query


def box_resize(img, out):
    """PIL's 8-bit BOX resample of a square uint8 image through the coefficient tables: horizontal pass first, 8-bit
    intermediate, 22-bit fixed point with rounding, as vk_preprocess_kernel does it."""
    side = img.shape[0]
    bounds, coef = query.box_tables(side, out)

    def one_axis(a):   # a: [n_in, m] -> [out, m]
        res = np.empty((out, a.shape[1]), dtype=np.uint8)
        for i in range(out):
            x0, n = bounds[i]
            acc = (1 << 21) + (a[x0:x0 + n].astype(np.int64) * coef[i, :n, None]).sum(axis=0)
            res[i] = np.clip(acc >> 22, 0, 255)
        return res
    return one_axis(one_axis(img.T).T)


def resized_set(imgs, out):
    return np.stack([box_resize(im, out) for im in imgs])


def takes_partner(i, partner, lam, rect, mode):
    """Does row i use any value of its partner?  Not in mode 0, with itself as partner, with lam == 1 (MixUp) or an
    empty rectangle (CutMix)."""
    x1, y1, x2, y2 = rect
    if mode == 0 or int(partner[i]) == i:
        return False
    return float(lam[i]) != 1.0 if mode == 1 else (x2 > x1 and y2 > y1)


def is_lit(bshift, cscale):
    return float(bshift) != 0.0 or float(cscale) != 1.0


def batch_f64(resized, idx, partner, lam, bshift, cscale, rect, mode, mean=0.5, std=0.5):
    """float64 [B, 3, out, out] from the resized set uint8 [nset, out, out] (steps 2-8 of the rule)."""
    out = resized.shape[1]
    B = len(idx)

    def value(i):
        x = resized[idx[i]].astype(np.float64) / 255.0
        if is_lit(bshift[i], cscale[i]):
            x = np.clip(x, 1e-7, 1.0 - 1e-7)
            z = -np.log(1.0 / x - 1.0)
            x = 1.0 / (1.0 + np.exp(-((z + np.float64(bshift[i])) * np.float64(cscale[i]))))
        return (x - mean) / std
    res = np.empty((B, 3, out, out), dtype=np.float64)
    x1, y1, x2, y2 = rect
    for i in range(B):
        s = value(i)
        if takes_partner(i, partner, lam, rect, mode):
            sp = value(int(partner[i]))
            if mode == 1:
                s = np.float64(lam[i]) * s + (1.0 - np.float64(lam[i])) * sp
            else:
                s = s.copy()
                s[y1:y2, x1:x2] = sp[y1:y2, x1:x2]
        res[i] = s[None]
    return res


def batch_f32_torch(resized, idx, partner, lam, bshift, cscale, rect, mode, mean=0.5, std=0.5):
    """The same formula, operation by operation, in float32 torch ops on the CPU: float32 [B, 3, out, out]."""
    import torch
    r = torch.from_numpy(np.array(resized))   # (a copy: the caller's array may be read-only)
    B = len(idx)
    f32 = torch.float32
    lo, hi = torch.tensor(1e-7, dtype=f32), torch.tensor(1.0, dtype=f32) - torch.tensor(1e-7, dtype=f32)
    mean_t, std_t = torch.tensor(mean, dtype=f32), torch.tensor(std, dtype=f32)

    def value(i):
        x = r[int(idx[i])].to(f32) / torch.tensor(255.0, dtype=f32)
        if is_lit(bshift[i], cscale[i]):
            x = torch.minimum(torch.maximum(x, lo), hi)
            z = -torch.log(1.0 / x - 1.0)
            x = 1.0 / (1.0 + torch.exp(-((z + torch.tensor(float(bshift[i]), dtype=f32)) * torch.tensor(float(cscale[i]), dtype=f32))))
        return (x - mean_t) / std_t
    rows = []
    x1, y1, x2, y2 = rect
    for i in range(B):
        s = value(i)
        if takes_partner(i, partner, lam, rect, mode):
            sp = value(int(partner[i]))
            if mode == 1:
                l = torch.tensor(float(lam[i]), dtype=f32)
                s = l * s + (1.0 - l) * sp
            else:
                s = s.clone()
                s[y1:y2, x1:x2] = sp[y1:y2, x1:x2]
        rows.append(s[None].expand(3, -1, -1))
    return torch.stack(rows).numpy()


def asymmetric_loss_f64(logits, y, gamma_neg=4.0, gamma_pos=0.0, clip=0.1, eps=1e-2):
    """The formula of train.asymmetric_loss's docstring in numpy float64."""
    logits, y = np.asarray(logits, dtype=np.float64), np.asarray(y, dtype=np.float64)
    p = 1.0 / (1.0 + np.exp(-logits))
    m = np.minimum(1.0 - p + clip, 1.0)
    loss = y * np.log(np.maximum(p, eps)) + (1.0 - y) * np.log(np.maximum(m, eps))
    w = (1.0 - (p * y + m * (1.0 - y))) ** (gamma_pos * y + gamma_neg * (1.0 - y))
    return float(-(w * loss).sum())
