"""torchvision.ops.deform_conv2d restated in torch on the CPU (unpinned: the torchvision source is absent), for the tests of
fasterrcnn_amd.ops.deform_conv2d: the operator from its contract (fasterrcnn_amd/ops.py's docstring) with floor, index gathers and
einsum -- dtype-generic and differentiable by autograd --, its five gradients written out explicitly with torchvision's
get_coordinate_weight, and the maker of the test cases."""
import torch

# (N, C_in, C_out, groups, G, kernel, stride, padding, dilation, H, W): the smallest geometries at which each index can go wrong
GEOMETRIES = [
    (3, 8, 6, 2, 2, (3, 3), (1, 1), (1, 1), (1, 1), 9, 11),     # 99 outputs per image: an odd row length
    (2, 4, 5, 1, 4, (3, 2), (1, 2), (1, 0), (1, 2), 10, 7),     # odd C_out; non-square kernel, stride, padding and dilation
    (3, 6, 6, 3, 1, (1, 1), (1, 1), (0, 0), (1, 1), 9, 11),     # 1x1 kernel, G < groups
    (1, 12, 8, 4, 2, (3, 3), (2, 1), (2, 1), (2, 1), 12, 9),    # G and groups do not nest channel-for-channel
    (2, 3, 2, 1, 3, (2, 3), (1, 1), (0, 1), (1, 1), 8, 8),      # one channel per offset group
]


def output_size(h, w, kernel, stride, padding, dilation):
    oh = (h + 2 * padding[0] - (dilation[0] * (kernel[0] - 1) + 1)) // stride[0] + 1
    ow = (w + 2 * padding[1] - (dilation[1] * (kernel[1] - 1) + 1)) // stride[1] + 1
    return oh, ow


def positions(offset, kernel, stride, padding, dilation):
    """The sample coordinates (y, x), each [N, G, kh kw, oh, ow]: the integer position first, then the displacement."""
    n, ch, oh, ow = offset.shape
    kh, kw = kernel
    off = offset.reshape(n, ch // (2 * kh * kw), kh * kw, 2, oh, ow)
    dev = offset.device
    tap_i = torch.arange(kh, device=dev).repeat_interleave(kw) * dilation[0]
    tap_j = torch.arange(kw, device=dev).repeat(kh) * dilation[1]
    base_y = (torch.arange(oh, device=dev) * stride[0] - padding[0])[None, :, None] + tap_i[:, None, None]        # [kk, oh, 1]
    base_x = (torch.arange(ow, device=dev) * stride[1] - padding[1])[None, None, :] + tap_j[:, None, None]        # [kk, 1, ow]
    return base_y.to(offset.dtype) + off[:, :, :, 0], base_x.to(offset.dtype) + off[:, :, :, 1]


class Corners:
    """floor / floor + 1 of the sample coordinates: the four corner indices, their in-map flags, the fractions and the values."""

    def __init__(self, input, y, x):
        n, c, h, w = input.shape
        g = y.shape[1]
        self.shape = (n, g, c // g) + tuple(y.shape[2:])                     # [N, G, C / G, kk, oh, ow]
        yl, xl = torch.floor(y.detach()), torch.floor(x.detach())
        self.lh, self.lw = y - yl, x - xl
        self.hh, self.hw_ = 1 - self.lh, 1 - self.lw
        self.accepted = (y > -1) & (y < h) & (x > -1) & (x < w)
        yi, xi = yl.long(), xl.long()
        self.index, self.inside = [], []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            cy, cx = yi + dy, xi + dx
            self.inside.append((cy >= 0) & (cy <= h - 1) & (cx >= 0) & (cx <= w - 1))
            self.index.append(cy.clamp(0, h - 1) * w + cx.clamp(0, w - 1))
        planes = input.reshape(n, g, c // g, h * w)
        self.values = [self.gather(planes, i) * k.unsqueeze(2) for i, k in zip(self.index, self.inside)]

    def gather(self, planes, index):
        n, g, cpo = self.shape[:3]
        idx = index.reshape(n, g, 1, -1).expand(n, g, cpo, -1)
        return torch.gather(planes, 3, idx).reshape(self.shape)

    def weights(self):
        return [self.hh * self.hw_, self.hh * self.lw, self.lh * self.hw_, self.lh * self.lw]

    def sample(self):
        """bilinear_interpolate: [N, G, C / G, kk, oh, ow]; 0 for a rejected sample."""
        w, v = [t.unsqueeze(2) for t in self.weights()], self.values
        val = w[0] * v[0] + w[1] * v[1] + w[2] * v[2] + w[3] * v[3]
        return val * self.accepted.unsqueeze(2)

    def coordinate_weight(self, y_direction):
        """get_coordinate_weight: no early-out -- only the corners' own validity."""
        v_yx, v_yX, v_Yx, v_YX = self.values
        if y_direction:
            return self.lw.unsqueeze(2) * (v_YX - v_yX) + self.hw_.unsqueeze(2) * (v_Yx - v_yx)
        return self.lh.unsqueeze(2) * (v_YX - v_Yx) + self.hh.unsqueeze(2) * (v_yX - v_yx)


def _columns(input, offset, mask, kernel, stride, padding, dilation):
    y, x = positions(offset, kernel, stride, padding, dilation)
    corners = Corners(input, y, x)
    sample = corners.sample()
    col = sample if mask is None else mask.reshape(sample.shape[:2] + (1,) + sample.shape[3:]) * sample
    return corners, sample, col


def deform_conv2d_ref(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    n, c = input.shape[:2]
    co, cg, kh, kw = weight.shape
    groups = c // cg
    _, _, col = _columns(input, offset, mask, (kh, kw), stride, padding, dilation)
    oh, ow = col.shape[-2:]
    col = col.reshape(n, groups, cg, kh * kw, oh * ow)
    out = torch.einsum("gock,ngckp->ngop", weight.reshape(groups, co // groups, cg, kh * kw), col).reshape(n, co, oh, ow)
    return out if bias is None else out + bias[None, :, None, None]


def deform_conv2d_grads_ref(input, offset, weight, bias, stride, padding, dilation, mask, grad):
    """(d_input, d_offset, d_weight, d_bias, d_mask) written out, in the dtype of the arguments (float64 in the tests); d_bias / d_mask are
    None without bias / mask."""
    n, c, h, w = input.shape
    co, cg, kh, kw = weight.shape
    groups, kk = c // cg, kh * kw
    corners, sample, col = _columns(input, offset, mask, (kh, kw), stride, padding, dilation)
    g = sample.shape[1]
    oh, ow = sample.shape[-2:]
    grad_g = grad.reshape(n, groups, co // groups, oh * ow)
    w_g = weight.reshape(groups, co // groups, cg, kk)
    d_weight = torch.einsum("ngop,ngckp->gock", grad_g, col.reshape(n, groups, cg, kk, oh * ow)).reshape(weight.shape)
    d_bias = None if bias is None else grad.sum((0, 2, 3))
    dcol = torch.einsum("gock,ngop->ngckp", w_g, grad_g).reshape(n, g, c // g, kk, oh, ow)
    m = torch.ones_like(sample[:, :, :1]) if mask is None else mask.reshape(n, g, 1, kk, oh, ow)
    d_mask = None if mask is None else (dcol * sample).sum(2).reshape(mask.shape)
    d_y = (m * corners.coordinate_weight(True) * dcol).sum(2)
    d_x = (m * corners.coordinate_weight(False) * dcol).sum(2)
    d_offset = torch.stack([d_y, d_x], dim=3).reshape(offset.shape)
    d_input = torch.zeros((n, g, c // g, h * w), dtype=input.dtype, device=input.device)
    for wk, index, inside in zip(corners.weights(), corners.index, corners.inside):
        term = (wk * (inside & corners.accepted)).unsqueeze(2) * m * dcol
        idx = index.reshape(n, g, 1, -1).expand(n, g, c // g, -1)
        d_input.scatter_add_(3, idx, term.reshape(n, g, c // g, -1))
    return d_input.reshape(input.shape), d_offset, d_weight, d_bias, d_mask


def border_shares(input_shape, offset, kernel, stride, padding, dilation):
    """(share of samples rejected outright, share accepted with at least one corner outside the map)."""
    h, w = input_shape[2:]
    y, x = positions(offset, kernel, stride, padding, dilation)
    accepted = (y > -1) & (y < h) & (x > -1) & (x < w)
    yl, xl = torch.floor(y), torch.floor(x)
    whole = (yl >= 0) & (yl + 1 <= h - 1) & (xl >= 0) & (xl + 1 <= w - 1)
    return float((~accepted).double().mean()), float((accepted & ~whole).double().mean())


def make_case(geometry, seed, with_mask=True, with_bias=True, offset_sigma=2.0):
    """Float32 tensors from a fixed seed: values randn, offsets N(0, offset_sigma px), mask U(0, 1).  A dict with the arguments, the
    output gradient `grad`, the keyword geometry `kw` and the two border shares."""
    n, c, co, groups, g, kernel, stride, padding, dilation, h, w = geometry
    gen = torch.Generator().manual_seed(seed)
    oh, ow = output_size(h, w, kernel, stride, padding, dilation)
    kk = kernel[0] * kernel[1]
    case = {
        "input": torch.randn((n, c, h, w), generator=gen),
        "offset": torch.randn((n, 2 * g * kk, oh, ow), generator=gen) * offset_sigma,
        "weight": torch.randn((co, c // groups) + tuple(kernel), generator=gen),
        "bias": torch.randn((co,), generator=gen) if with_bias else None,
        "mask": torch.rand((n, g * kk, oh, ow), generator=gen) if with_mask else None,
        "grad": torch.randn((n, co, oh, ow), generator=gen),
        "kw": {"stride": stride, "padding": padding, "dilation": dilation},
    }
    case["rejected"], case["straddling"] = border_shares(case["input"].shape, case["offset"], kernel, stride, padding, dilation)
    return case


ARGS = ("input", "offset", "weight", "bias", "mask")


def cast(case, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def forward_ref(case, dtype):
    c = cast(case, dtype)
    return deform_conv2d_ref(c["input"], c["offset"], c["weight"], c["bias"], mask=c["mask"], **c["kw"])


def grads_ref(case, dtype):
    c = cast(case, dtype)
    kw = c["kw"]
    return deform_conv2d_grads_ref(c["input"], c["offset"], c["weight"], c["bias"], kw["stride"], kw["padding"], kw["dilation"], c["mask"],
                                   c["grad"])


def autograd_ref(case, dtype):
    """The five gradients by autograd through deform_conv2d_ref."""
    c = cast(case, dtype)
    leaves = [c[k].clone().requires_grad_(True) if c[k] is not None else None for k in ARGS]
    out = deform_conv2d_ref(leaves[0], leaves[1], leaves[2], leaves[3], mask=leaves[4], **c["kw"])
    out.backward(c["grad"])
    return tuple(None if t is None else t.grad for t in leaves)


def rel_err(a, truth):
    """max |a - truth| / max |truth|"""
    return float((a.double() - truth.double()).abs().max() / truth.double().abs().max())
