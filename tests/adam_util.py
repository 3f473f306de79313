"""Shared by the Adam tests: fixed gradient sequences, the torch.optim oracle and the error measure."""
import torch

LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-7
STEPS = 5


def fixed_grads(store, steps=STEPS, seed=7):
    """``steps`` flat gradient buffers (CPU fp32): N(0, 1) values on the parameters' elements, 0 on the
    alignment padding; in every tensor elements 1::7 are exactly 0 and elements 2::7 are ~1e-20 (g * g
    underflows fp32's normal range)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        flat = torch.zeros(store.total, dtype=torch.float32)
        for s in store.specs:
            v = torch.randn(s.numel, generator=g)
            v[1::7] = 0.0
            v[2::7] = 1e-20 * (1.0 + torch.rand(v[2::7].numel(), generator=g))
            flat[store.offsets[s.name]: store.offsets[s.name] + s.numel] = v
        out.append(flat)
    return out


def valid_mask(store):
    m = torch.zeros(store.total, dtype=torch.bool)
    for s in store.specs:
        m[store.offsets[s.name]: store.offsets[s.name] + s.numel] = True
    return m


def torch_adam(w0, grads, name, weight_decay, grad_scale, dtype):
    """torch.optim.Adam (L2 weight decay) / AdamW (decoupled) on the fp32 inputs ``w0`` / ``grads`` cast to
    ``dtype``; the gradient handed to it is grad_scale * grad.  Returns the per-step histories
    {"w": [w0, w1, ...], "m": [0, m1, ...], "v": [0, v1, ...]}."""
    p = torch.nn.Parameter(w0.detach().cpu().to(dtype).clone())
    cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    opt = cls([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    hist = {"w": [p.detach().clone()], "m": [torch.zeros_like(p)], "v": [torch.zeros_like(p)]}
    for g in grads:
        p.grad = g.to(dtype) * grad_scale
        opt.step()
        st = opt.state[p]
        hist["w"].append(p.detach().clone())
        hist["m"].append(st["exp_avg"].clone())
        hist["v"].append(st["exp_avg_sq"].clone())
    return hist


def rel_err(x, ref_hist):
    """Maximum over the elements of |x - ref| / scale, ref = the oracle's final value and scale = the
    largest magnitude the oracle's element took over the run (never below 1e-30).

    Relative to the final value alone the measure is ill-conditioned wherever an update cancels: w - upd
    that lands near 0 carries the absolute rounding error of its operands, in any fp32 implementation.
    The operands' magnitude is the scale fp32 rounding is proportional to.  The 1e-30 guard keeps
    elements that are exactly 0 (and the denormal second moments of the ~1e-20 gradients, whose absolute
    error is at most 1.4e-45) from dividing by nothing."""
    ref = ref_hist[-1].double()
    scale = torch.stack([h.double().abs() for h in ref_hist]).amax(dim=0).clamp_min(1e-30)
    return float(((x.detach().cpu().double() - ref).abs() / scale).max())
