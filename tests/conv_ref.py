"""The CNN height-map encoder's convolution stack (rollout_cnn.HeightMapEncoder with use_cnn: Conv 3x3 pad 1, ReLU,
MaxPool 2, twice, on the (2, 61, 31) map) restated in plain torch for the tests of csrc/ppo_conv.h: the stack and its
autograd gradients in any precision, the rows on which exact ties decide, and the decision screen.

The screen.  A pool winner or a ReLU sign that is decided within rounding makes a 3xF16 result and the f64 reference
differ by a whole term, which no tolerance covers; so rows are screened, as a condition on the inputs.  In f64 every
pre-activation z gets an error bound: conv1 2^-21 (|W| * |x| + |b|); conv2 the same on its own operands plus
|W2| * (conv1's bound after pooling: the window's largest).  A row is unsafe if, in any window, the winner is within
MARGIN x the summed bounds of another candidate while it could pass the ReLU (winner > -MARGIN x its bound), or the
winner is within MARGIN x its bound of zero.  Candidates whose input patches are bit-identical are exempt: any
implementation computes them identically and the tie rule (the first maximum in the order (0,0) (0,1) (1,0) (1,1),
ReLU'(0) = 0) decides, which is what the tie rows are for.  Unsafe rows are redrawn from the seeded stream.
"""
import torch
import torch.nn.functional as F

MAP = (2, 61, 31)
N_MAP, N_FEAT = 2 * 61 * 31, 32 * 15 * 7
EPS = 2.0 ** -21   # the 3xF16 product's relative error
MARGIN = 4.0
NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")


def make_filters(gen, device="cpu"):
    """(w1, b1, w2, b2) f32: weights U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), biases U(-0.1, 0.1) (tests/cnn_cases.py)."""
    out = []
    for shape in ((16, 2, 3, 3), (32, 16, 3, 3)):
        b = 1.0 / (shape[1] * 9) ** 0.5
        out.append(((torch.rand(shape, generator=gen) * 2 - 1) * b).to(device))
        out.append(((torch.rand(shape[0], generator=gen) * 2 - 1) * 0.1).to(device))
    return out


def draw_maps(gen, n):
    """(n, 3782) f32 map values U(-5, 5) (tests/cnn_cases.py's recipe)."""
    return torch.rand(n, N_MAP, generator=gen) * 10.0 - 5.0


def tie_maps():
    """Three rows on which exact ties decide: a map constant per channel, a map of two integer plateaus, all zeros."""
    const = torch.empty(MAP)
    const[0], const[1] = 1.5, -0.75
    plat = torch.zeros(MAP)
    plat[0, :, 16:] = 2.0
    plat[0, 31:, :] = 3.0
    plat[1, :40] = -1.0
    plat[1, 40:] = 4.0
    return torch.stack([const.reshape(-1), plat.reshape(-1), torch.zeros(N_MAP)])


def stack(maps, w1, b1, w2, b2, keep=None):
    """The features (n, 3360) of maps (n, 3782); `keep`: a dict that receives the pre-activations z1, z2."""
    x = maps.reshape(-1, *MAP)
    z1 = F.conv2d(x, w1, b1, padding=1)
    z2 = F.conv2d(F.max_pool2d(F.relu(z1), 2), w2, b2, padding=1)
    if keep is not None:
        keep.update(z1=z1, z2=z2)
    return F.max_pool2d(F.relu(z2), 2).flatten(1)


def grads(maps, filters, d_feat, dtype):
    """feat and the autograd gradients of sum(feat * d_feat) in `dtype`: (feat, [dW1, db1, dW2, db2], row_terms);
    row_terms: the per-pixel terms of the two bias gradients, which are plain sums (tests/ppo_cases._compare)."""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in filters]
    keep = {}
    feat = stack(maps.to(dtype), *ps, keep=keep)
    g = torch.autograd.grad((feat * d_feat.to(dtype)).sum(), ps + [keep["z1"], keep["z2"]])
    terms = {"conv1.bias": g[4].permute(0, 2, 3, 1).reshape(-1, 16), "conv2.bias": g[5].permute(0, 2, 3, 1).reshape(-1, 32)}
    return feat.detach(), [t.detach() for t in g[:4]], terms


def _windows(t):
    """(n, C, X, Y) -> (n, C, X // 2, Y // 2, 4): the pool windows' candidates in torch's scan order."""
    n, c, X, Y = t.shape
    px, py = X // 2, Y // 2
    return t[:, :, :2 * px, :2 * py].reshape(n, c, px, 2, py, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, px, py, 4)


def _stage(z, e, src):
    """Unsafe rows of one conv -> ReLU -> pool stage: z the pre-activations, e their bounds, src the conv's input."""
    n, C = z.shape[:2]
    zw, ew = _windows(z), _windows(e)
    best, arg = zw[..., 0], torch.zeros_like(zw[..., 0], dtype=torch.long)
    for j in (1, 2, 3):  # torch's rule: replaced only on strictly greater
        up = zw[..., j] > best
        best, arg = torch.where(up, zw[..., j], best), torch.where(up, j, arg)
    ebest = ew.gather(-1, arg[..., None])[..., 0]
    pw = _windows(F.unfold(src, 3, padding=1).reshape(n, -1, *z.shape[2:]))  # (n, K, px, py, 4): the patches
    unsafe = best.abs() < MARGIN * ebest
    could_pass = best > -MARGIN * ebest
    for j in range(4):
        close = (best - zw[..., j] <= MARGIN * (ebest + ew[..., j])) & (arg != j) & could_pass
        if not bool(close.any()):
            continue
        # exempt where candidate j's patch equals the winner's, bit for bit
        pwin = pw.unsqueeze(1).expand(n, C, *pw.shape[1:]).gather(-1, arg[:, :, None, :, :, None].expand(
            n, C, pw.shape[1], *arg.shape[2:], 1))[..., 0]  # (n, C, K, px, py)
        same = (pwin == pw[..., j].unsqueeze(1)).all(2)
        unsafe = unsafe | (close & ~same)
    return unsafe.flatten(1).any(1)


def unsafe_rows(maps, w1, b1, w2, b2):
    """The screen of the module docstring on maps (n, 3782): a bool per row.  Computed in f64 wherever the inputs live."""
    with torch.no_grad():
        x = maps.double().reshape(-1, *MAP)
        w1, b1, w2, b2 = (t.detach().double() for t in (w1, b1, w2, b2))
        out = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
        for lo in range(0, x.shape[0], 16):  # the conv2 patches of a row are 0.5 MB
            xs = x[lo:lo + 16]
            z1 = F.conv2d(xs, w1, b1, padding=1)
            e1 = EPS * F.conv2d(xs.abs(), w1.abs(), b1.abs(), padding=1)
            u1 = _stage(z1, e1, xs)
            p1, pe1 = F.max_pool2d(F.relu(z1), 2), F.max_pool2d(e1, 2)
            z2 = F.conv2d(p1, w2, b2, padding=1)
            e2 = EPS * F.conv2d(p1, w2.abs(), b2.abs(), padding=1) + F.conv2d(pe1, w2.abs(), None, padding=1)
            out[lo:lo + 16] = u1 | _stage(z2, e2, p1)
        return out


def screened_maps(gen, n, filters, rounds=40):
    """n rows of draw_maps with every unsafe row redrawn from the same stream until none is left (AssertionError
    after `rounds`: the screen must converge).  Returns (maps, rounds used, unsafe rows of the first round)."""
    maps = draw_maps(gen, n)
    first = None
    for r in range(rounds):
        bad = unsafe_rows(maps.to(filters[0].device), *filters).cpu()
        first = int(bad.sum()) if first is None else first
        if not bool(bad.any()):
            return maps, r, first
        maps[bad] = draw_maps(gen, int(bad.sum()))
    raise AssertionError(f"the decision screen did not converge in {rounds} rounds")
