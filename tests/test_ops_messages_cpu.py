"""The full text of the argument errors of fasterrcnn_amd.ops' sampler operators, without a GPU: dcnv3, dcnv4, DCNv3Function.apply,
DCNv4Function.apply, multi_scale_deformable_attn, carafe's integer rules and the callers of the int-or-pair rule (deform_conv2d and
DeformConv2d included).  One literal table: the arguments that differ from a valid call on meta tensors, the exception type and the
whole message, compared with ==; the per-operator tests match fragments only.  The rows that break two rules at once pin the order of
the checks.  The 32-bit index rules need large shape numbers only: a meta tensor owns no memory."""
import pytest
import torch

from fasterrcnn_amd import ops

F16, BF16, F32, F64, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
NO_CPU = ": fasterrcnn_amd.ops has no CPU implementation"
LOWER = " (lower im2col_step)"


def M(*shape, dtype=F32, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


# ---- the valid calls: the smallest shapes that reach every rule ---------------------------------------------------------------------
def call_dcnv3(**kw):
    a = dict(input=M(1, 3, 3, 2), offset=M(1, 1, 1, 18), mask=M(1, 1, 1, 9), kernel_size=3)
    a.update(kw)
    return ops.dcnv3(**a)


def call_dcnv4(**kw):
    a = dict(input=M(1, 3, 3, 2), offset_mask=M(1, 1, 1, 32), kernel_size=3)
    a.update(kw)
    return ops.dcnv4(**a)


_FUNCTION = dict(kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_h=0, pad_w=0, dilation_h=1, dilation_w=1, group=1, group_channels=2,
                 offset_scale=1.0, im2col_step=256)


def call_dcnv3_function(**kw):
    a = dict(input=M(1, 3, 3, 2), offset=M(1, 1, 1, 18), mask=M(1, 1, 1, 9), **_FUNCTION)
    a.update(kw)
    return ops.DCNv3Function.apply(*a.values())             # positional, in upstream's order


def call_dcnv4_function(**kw):
    a = dict(input=M(1, 3, 3, 2), offset_mask=M(1, 1, 1, 32), **_FUNCTION, remove_center=False)
    a.update(kw)
    return ops.DCNv4Function.apply(*a.values())


def _msda_args(kw):
    a = dict(value=M(1, 4, 1, 2), value_spatial_shapes=M(1, 2, dtype=I64), value_level_start_index=M(1, dtype=I64),
             sampling_locations=M(1, 1, 1, 1, 1, 2), attention_weights=M(1, 1, 1, 1, 1))
    a.update(kw)
    return a


def call_msda(**kw):
    return ops.multi_scale_deformable_attn(**_msda_args(kw))


def call_msda_function(**kw):
    a = _msda_args(kw)
    step = a.pop("im2col_step", 64)
    return ops.MultiScaleDeformableAttnFunction.apply(*a.values(), step)


def call_carafe(**kw):
    a = dict(features=M(1, 2, 2, 2), masks=M(1, 9, 2, 2), kernel_size=3, group_size=1, scale_factor=1)
    a.update(kw)
    return ops.carafe(**a)


def call_deform_conv2d(**kw):
    a = dict(input=M(1, 2, 3, 3), offset=M(1, 18, 1, 1), weight=M(2, 2, 3, 3))
    a.update(kw)
    return ops.deform_conv2d(**a)


def call_deform_module(**kw):
    a = dict(in_channels=2, out_channels=2, kernel_size=3)
    a.update(kw)
    return ops.DeformConv2d(**a)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
LEVELS9 = dict(sampling_locations=M(1, 1, 1, 9, 1, 2), attention_weights=M(1, 1, 1, 9, 1), value_spatial_shapes=M(9, 2, dtype=I64),
               value_level_start_index=M(9, dtype=I64))

TABLE = [
    # dcnv3(): the pairs, then group, then the shared rules
    (call_dcnv3, dict(kernel_size=3.0), TypeError, "kernel_size must be an int or a pair of ints, got 3.0"),
    (call_dcnv3, dict(kernel_size=True), TypeError, "kernel_size must be an int or a pair of ints, got True"),
    (call_dcnv3, dict(kernel_size=(3, 3, 3)), TypeError, "kernel_size must be an int or a pair of ints, got (3, 3, 3)"),
    (call_dcnv3, dict(kernel_size=[3, False]), TypeError, "kernel_size must be an int or a pair of ints, got [3, False]"),
    (call_dcnv3, dict(kernel_size=0), ValueError, "kernel_size must be >= 1, got (0, 0)"),
    (call_dcnv3, dict(stride="1"), TypeError, "stride must be an int or a pair of ints, got '1'"),
    (call_dcnv3, dict(stride=(1, 0)), ValueError, "stride must be >= 1, got (1, 0)"),
    (call_dcnv3, dict(padding=None), TypeError, "padding must be an int or a pair of ints, got None"),
    (call_dcnv3, dict(padding=-1), ValueError, "padding must be >= 0, got (-1, -1)"),
    (call_dcnv3, dict(dilation=1.0), TypeError, "dilation must be an int or a pair of ints, got 1.0"),
    (call_dcnv3, dict(dilation=[0, 1]), ValueError, "dilation must be >= 1, got (0, 1)"),
    (call_dcnv3, dict(group=1.0), TypeError, "group must be an int, got 1.0"),
    (call_dcnv3, dict(group=True), TypeError, "group must be an int, got True"),
    (call_dcnv3, dict(group=0), ValueError, "group must be at least 1, got 0"),
    (call_dcnv3, dict(input=M(1, 3, 3, 3), group=2), ValueError, "input's 3 channels must be divisible by group, got 2"),
    (call_dcnv3, dict(input=None), TypeError, "input must be a torch.Tensor, got NoneType"),
    (call_dcnv3, dict(input=M(1, 3, 3, 2, dtype=F64)), TypeError, "input must be float32, float16 or bfloat16, got torch.float64"),
    (call_dcnv3, dict(input=M(1, 3, 3, 2, device="cpu")), ValueError, "input must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_dcnv3, dict(offset=[1]), TypeError, "offset must be a torch.Tensor, got list"),
    (call_dcnv3, dict(offset=M(1, 1, 1, 18, dtype=F16)), TypeError, "offset must be float32, got torch.float16"),
    (call_dcnv3, dict(input=M(1, 3, 3, 2, dtype=F16), offset=M(1, 1, 1, 18, dtype=BF16)), TypeError,
     "offset must be float32 or the input's torch.float16, got torch.bfloat16"),
    (call_dcnv3, dict(offset=M(1, 1, 1, 18, device="cpu")), ValueError, "offset must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_dcnv3, dict(mask=M(1, 1, 1, 9, dtype=F64)), TypeError, "mask must be float32, got torch.float64"),
    (call_dcnv3, dict(input=M(1, 3, 3, 2, dtype=BF16), mask=M(1, 1, 1, 9, dtype=F16)), TypeError,
     "mask must be float32 or the input's torch.bfloat16, got torch.float16"),
    (call_dcnv3, dict(mask=M(1, 1, 1, 9, device="cpu")), ValueError, "mask must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_dcnv3, dict(input=M(3, 3, 2)), ValueError, "input must be [N, H, W, C] (channels last), got shape (3, 3, 2)"),
    (call_dcnv3, dict(im2col_step=256.0), TypeError, "im2col_step must be an int, got 256.0"),
    (call_dcnv3, dict(im2col_step=True), TypeError, "im2col_step must be an int, got True"),
    (call_dcnv3, dict(offset_scale="1"), TypeError, "offset_scale must be a float, got '1'"),
    (call_dcnv3, dict(offset_scale=True), TypeError, "offset_scale must be a float, got True"),
    (call_dcnv3, dict(offset_scale=float("inf")), ValueError, "offset_scale must be finite, got inf"),
    (call_dcnv3, dict(offset_scale=float("nan")), ValueError, "offset_scale must be finite, got nan"),
    (call_dcnv3, dict(im2col_step=0), ValueError, "im2col_step must be at least 1, got 0"),
    (call_dcnv3, dict(input=M(1, 3, 3, 257)), ValueError, "group_channels must lie in [1, MAX_DCNV3_CHANNELS = 256], got 257"),
    (call_dcnv3, dict(input=M(1, 3, 3, 0)), ValueError, "group_channels must lie in [1, MAX_DCNV3_CHANNELS = 256], got 0"),
    (call_dcnv3, dict(kernel_size=8), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (8, 8)"),
    (call_dcnv3, dict(kernel_size=(3, 9)), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (3, 9)"),
    (call_dcnv3, dict(stride=65537), ValueError, "stride must lie in [1, MAX_DCNV3_STEP = 65536], got (65537, 65537)"),
    (call_dcnv3, dict(padding=(0, 65537)), ValueError, "padding must lie in [0, MAX_DCNV3_STEP = 65536], got (0, 65537)"),
    (call_dcnv3, dict(dilation=(65537, 1)), ValueError, "dilation must lie in [1, MAX_DCNV3_STEP = 65536], got (65537, 1)"),
    (call_dcnv3, dict(input=M(1, 2 ** 24 + 1, 3, 2)), ValueError,
     "input must have H and W of at most MAX_DCNV3_SIDE = 16777216, got shape (1, 16777217, 3, 2)"),
    (call_dcnv3, dict(offset=M(1, 1, 1, 17)), ValueError, "offset must be [N, Ho, Wo, G K 2] = [1, 1, 1, 18], got shape (1, 1, 1, 17)"),
    (call_dcnv3, dict(offset=M(1, 18, 1, 1)), ValueError, "offset must be [N, Ho, Wo, G K 2] = [1, 1, 1, 18], got shape (1, 18, 1, 1)"),
    (call_dcnv3, dict(mask=M(1, 1, 1, 8)), ValueError, "mask must be [N, Ho, Wo, G K] = [1, 1, 1, 9], got shape (1, 1, 1, 8)"),
    (call_dcnv3, dict(input=M(1, 4, 3, 2), padding=1, stride=2), ValueError,
     "offset must be [N, Ho, Wo, G K 2] = [1, 2, 2, 18], got shape (1, 1, 1, 18)"),
    (call_dcnv3, dict(input=M(1, 2 ** 16, 2 ** 16, 2), kernel_size=1, stride=65536, offset=M(1, 1, 1, 2), mask=M(1, 1, 1, 1)), ValueError,
     "input is too large for the kernels' 32-bit cell indices: 1 images x H x W x G = 4294967296 > MAX_MSDA_INDEX = 2147482623" + LOWER),
    (call_dcnv3, dict(input=M(1, 2 ** 15, 2 ** 15, 2), kernel_size=1, offset=M(1, 2 ** 15, 2 ** 15, 2), mask=M(1, 2 ** 15, 2 ** 15, 1)),
     ValueError, "offset is too large for the kernels' 32-bit plan indices: 1 images x Ho x Wo x G x K x 4 = 4294967296 > MAX_MSDA_INDEX = "
     "2147482623" + LOWER),
    # DCNv3Function.apply: its own names for the pairs, and the rules dcnv3() decides before the shared ones
    (call_dcnv3_function, dict(kernel_h=3.0), TypeError, "kernel_h, kernel_w must be an int or a pair of ints, got (3.0, 3)"),
    (call_dcnv3_function, dict(kernel_w=0), ValueError, "kernel_h, kernel_w must be >= 1, got (3, 0)"),
    (call_dcnv3_function, dict(stride_w=True), TypeError, "stride_h, stride_w must be an int or a pair of ints, got (1, True)"),
    (call_dcnv3_function, dict(stride_h=0), ValueError, "stride_h, stride_w must be >= 1, got (0, 1)"),
    (call_dcnv3_function, dict(pad_h=None), TypeError, "pad_h, pad_w must be an int or a pair of ints, got (None, 0)"),
    (call_dcnv3_function, dict(pad_w=-1), ValueError, "pad_h, pad_w must be >= 0, got (0, -1)"),
    (call_dcnv3_function, dict(dilation_h="1"), TypeError, "dilation_h, dilation_w must be an int or a pair of ints, got ('1', 1)"),
    (call_dcnv3_function, dict(dilation_w=0), ValueError, "dilation_h, dilation_w must be >= 1, got (1, 0)"),
    (call_dcnv3_function, dict(group=1.0), TypeError, "group must be an int, got 1.0"),
    (call_dcnv3_function, dict(group_channels=2.0), TypeError, "group_channels must be an int, got 2.0"),
    (call_dcnv3_function, dict(group_channels=True), TypeError, "group_channels must be an int, got True"),
    (call_dcnv3_function, dict(im2col_step=None), TypeError, "im2col_step must be an int, got None"),
    (call_dcnv3_function, dict(group=0), ValueError, "group must be at least 1, got 0"),
    (call_dcnv3_function, dict(group=-2, group_channels=-1), ValueError, "group must be at least 1, got -2"),
    (call_dcnv3_function, dict(group_channels=3), ValueError,
     "group * group_channels must equal input's 2 channels, got group 1 and group_channels 3"),
    (call_dcnv3_function, dict(group=2, group_channels=2), ValueError,
     "group * group_channels must equal input's 2 channels, got group 2 and group_channels 2"),
    (call_dcnv3_function, dict(kernel_h=8), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (8, 3)"),
    (call_dcnv3_function, dict(pad_h=65537), ValueError, "padding must lie in [0, MAX_DCNV3_STEP = 65536], got (65537, 0)"),
    (call_dcnv3_function, dict(mask=M(1, 1, 1, 18)), ValueError, "mask must be [N, Ho, Wo, G K] = [1, 1, 1, 9], got shape (1, 1, 1, 18)"),
    # dcnv4(): dcnv3's rules on one tensor, remove_center, the record
    (call_dcnv4, dict(kernel_size=3.0), TypeError, "kernel_size must be an int or a pair of ints, got 3.0"),
    (call_dcnv4, dict(kernel_size=(0, 3)), ValueError, "kernel_size must be >= 1, got (0, 3)"),
    (call_dcnv4, dict(stride=0), ValueError, "stride must be >= 1, got (0, 0)"),
    (call_dcnv4, dict(padding=1.5), TypeError, "padding must be an int or a pair of ints, got 1.5"),
    (call_dcnv4, dict(dilation=0), ValueError, "dilation must be >= 1, got (0, 0)"),
    (call_dcnv4, dict(group=None), TypeError, "group must be an int, got None"),
    (call_dcnv4, dict(group=False), TypeError, "group must be an int, got False"),
    (call_dcnv4, dict(group=-1), ValueError, "group must be at least 1, got -1"),
    (call_dcnv4, dict(input=M(1, 3, 3, 5), group=4), ValueError, "input's 5 channels must be divisible by group, got 4"),
    (call_dcnv4, dict(input=3), TypeError, "input must be a torch.Tensor, got int"),
    (call_dcnv4, dict(input=M(1, 3, 3, 2, dtype=I32)), TypeError, "input must be float32, float16 or bfloat16, got torch.int32"),
    (call_dcnv4, dict(input=M(1, 3, 3, 2, device="cpu")), ValueError, "input must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_dcnv4, dict(offset_mask=None), TypeError, "offset_mask must be a torch.Tensor, got NoneType"),
    (call_dcnv4, dict(offset_mask=M(1, 1, 1, 32, dtype=BF16)), TypeError, "offset_mask must be float32, got torch.bfloat16"),
    (call_dcnv4, dict(input=M(1, 3, 3, 2, dtype=F16), offset_mask=M(1, 1, 1, 32, dtype=F64)), TypeError,
     "offset_mask must be float32 or the input's torch.float16, got torch.float64"),
    (call_dcnv4, dict(offset_mask=M(1, 1, 1, 32, device="cpu")), ValueError,
     "offset_mask must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_dcnv4, dict(input=M(1, 3, 3, 2, 1)), ValueError, "input must be [N, H, W, C] (channels last), got shape (1, 3, 3, 2, 1)"),
    (call_dcnv4, dict(im2col_step=1.5), TypeError, "im2col_step must be an int, got 1.5"),
    (call_dcnv4, dict(remove_center="yes"), TypeError, "remove_center must be a bool, got 'yes'"),
    (call_dcnv4, dict(remove_center=1.0), TypeError, "remove_center must be a bool, got 1.0"),
    (call_dcnv4, dict(remove_center=None), TypeError, "remove_center must be a bool, got None"),
    (call_dcnv4, dict(remove_center=2), ValueError, "remove_center must be False or True (0 or 1), got 2"),
    (call_dcnv4, dict(remove_center=-1), ValueError, "remove_center must be False or True (0 or 1), got -1"),
    (call_dcnv4, dict(offset_scale=None), TypeError, "offset_scale must be a float, got None"),
    (call_dcnv4, dict(offset_scale=False), TypeError, "offset_scale must be a float, got False"),
    (call_dcnv4, dict(offset_scale=float("-inf")), ValueError, "offset_scale must be finite, got -inf"),
    (call_dcnv4, dict(im2col_step=-3), ValueError, "im2col_step must be at least 1, got -3"),
    (call_dcnv4, dict(input=M(1, 3, 3, 514), group=2), ValueError, "group_channels must lie in [1, MAX_DCNV3_CHANNELS = 256], got 257"),
    (call_dcnv4, dict(kernel_size=(8, 1)), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (8, 1)"),
    (call_dcnv4, dict(kernel_size=(3, 5), remove_center=True), ValueError,
     "remove_center requires a square kernel of odd size >= 3, got (3, 5)"),
    (call_dcnv4, dict(kernel_size=2, remove_center=1), ValueError, "remove_center requires a square kernel of odd size >= 3, got (2, 2)"),
    (call_dcnv4, dict(kernel_size=1, remove_center=True), ValueError, "remove_center requires a square kernel of odd size >= 3, got (1, 1)"),
    (call_dcnv4, dict(stride=(1, 65537)), ValueError, "stride must lie in [1, MAX_DCNV3_STEP = 65536], got (1, 65537)"),
    (call_dcnv4, dict(padding=65537), ValueError, "padding must lie in [0, MAX_DCNV3_STEP = 65536], got (65537, 65537)"),
    (call_dcnv4, dict(dilation=65537), ValueError, "dilation must lie in [1, MAX_DCNV3_STEP = 65536], got (65537, 65537)"),
    (call_dcnv4, dict(input=M(1, 3, 2 ** 24 + 1, 2)), ValueError,
     "input must have H and W of at most MAX_DCNV3_SIDE = 16777216, got shape (1, 3, 16777217, 2)"),
    (call_dcnv4, dict(offset_mask=M(1, 1, 1, 27)), ValueError,
     "offset_mask must be [N, Ho, Wo, L] = [1, 1, 1, 32] with L = ceil(G P 3 / 8) 8 for G = 1 groups of P = 9 points (2 P offsets, then P "
     "masks; the record padded to a multiple of 8), got shape (1, 1, 1, 27)"),
    (call_dcnv4, dict(remove_center=True), ValueError,
     "offset_mask must be [N, Ho, Wo, L] = [1, 1, 1, 24] with L = ceil(G P 3 / 8) 8 for G = 1 groups of P = 8 points (2 P offsets, then P "
     "masks; the record padded to a multiple of 8), got shape (1, 1, 1, 32)"),
    (call_dcnv4, dict(group=2, dilation=2), ValueError,
     "offset_mask must be [N, Ho, Wo, L] = [1, 0, 0, 56] with L = ceil(G P 3 / 8) 8 for G = 2 groups of P = 9 points (2 P offsets, then P "
     "masks; the record padded to a multiple of 8), got shape (1, 1, 1, 32)"),
    (call_dcnv4, dict(input=M(1, 2 ** 16, 2 ** 16, 2), kernel_size=1, stride=65536, offset_mask=M(1, 1, 1, 8)), ValueError,
     "input is too large for the kernels' 32-bit cell indices: 1 images x H x W x G = 4294967296 > MAX_MSDA_INDEX = 2147482623" + LOWER),
    (call_dcnv4, dict(input=M(3, 2 ** 15, 2 ** 15, 2), kernel_size=1, stride=32768, offset_mask=M(3, 1, 1, 8), im2col_step=2), ValueError,
     "input is too large for the kernels' 32-bit cell indices: 2 images x H x W x G = 2147483648 > MAX_MSDA_INDEX = 2147482623" + LOWER),
    (call_dcnv4, dict(input=M(1, 2 ** 15, 2 ** 15, 2), kernel_size=1, offset_mask=M(1, 2 ** 15, 2 ** 15, 8)), ValueError,
     "offset_mask is too large for the kernels' 32-bit plan indices: 1 images x Ho x Wo x G x P x 4 = 4294967296 > MAX_MSDA_INDEX = "
     "2147482623" + LOWER),
    # DCNv4Function.apply
    (call_dcnv4_function, dict(kernel_w=None), TypeError, "kernel_h, kernel_w must be an int or a pair of ints, got (3, None)"),
    (call_dcnv4_function, dict(kernel_h=0), ValueError, "kernel_h, kernel_w must be >= 1, got (0, 3)"),
    (call_dcnv4_function, dict(stride_h=1.0), TypeError, "stride_h, stride_w must be an int or a pair of ints, got (1.0, 1)"),
    (call_dcnv4_function, dict(stride_w=0), ValueError, "stride_h, stride_w must be >= 1, got (1, 0)"),
    (call_dcnv4_function, dict(pad_w=False), TypeError, "pad_h, pad_w must be an int or a pair of ints, got (0, False)"),
    (call_dcnv4_function, dict(pad_h=-1), ValueError, "pad_h, pad_w must be >= 0, got (-1, 0)"),
    (call_dcnv4_function, dict(dilation_w=1.0), TypeError, "dilation_h, dilation_w must be an int or a pair of ints, got (1, 1.0)"),
    (call_dcnv4_function, dict(dilation_h=0), ValueError, "dilation_h, dilation_w must be >= 1, got (0, 1)"),
    (call_dcnv4_function, dict(group=True), TypeError, "group must be an int, got True"),
    (call_dcnv4_function, dict(group_channels=None), TypeError, "group_channels must be an int, got None"),
    (call_dcnv4_function, dict(im2col_step=False), TypeError, "im2col_step must be an int, got False"),
    (call_dcnv4_function, dict(remove_center=[]), TypeError, "remove_center must be a bool, got []"),
    (call_dcnv4_function, dict(remove_center=3), ValueError, "remove_center must be False or True (0 or 1), got 3"),
    (call_dcnv4_function, dict(group=0, group_channels=0), ValueError, "group must be at least 1, got 0"),
    (call_dcnv4_function, dict(group_channels=1), ValueError,
     "group * group_channels must equal input's 2 channels, got group 1 and group_channels 1"),
    (call_dcnv4_function, dict(kernel_h=5, kernel_w=3, remove_center=True), ValueError,
     "remove_center requires a square kernel of odd size >= 3, got (5, 3)"),
    (call_dcnv4_function, dict(offset_mask=M(1, 1, 1, 24)), ValueError,
     "offset_mask must be [N, Ho, Wo, L] = [1, 1, 1, 32] with L = ceil(G P 3 / 8) 8 for G = 1 groups of P = 9 points (2 P offsets, then P "
     "masks; the record padded to a multiple of 8), got shape (1, 1, 1, 24)"),
    # the DCN pair, two rules at once: the one that is checked first is raised
    (call_dcnv3, dict(group=True, stride=0), ValueError, "stride must be >= 1, got (0, 0)"),
    (call_dcnv3, dict(group=0, kernel_size=2.5), TypeError, "kernel_size must be an int or a pair of ints, got 2.5"),
    (call_dcnv3, dict(input=M(1, 3, 3, 3), group=2, offset=None), ValueError, "input's 3 channels must be divisible by group, got 2"),
    (call_dcnv3, dict(input=M(3, 3, 2), offset=M(1, 1, 1, 18, dtype=F64)), TypeError, "offset must be float32, got torch.float64"),
    (call_dcnv3, dict(offset=M(1, 1, 1, 17), mask=M(1, 1, 1, 8)), ValueError,
     "offset must be [N, Ho, Wo, G K 2] = [1, 1, 1, 18], got shape (1, 1, 1, 17)"),
    (call_dcnv3, dict(offset_scale="1", im2col_step=0), TypeError, "offset_scale must be a float, got '1'"),
    (call_dcnv3, dict(offset_scale=float("nan"), im2col_step=2.0), TypeError, "im2col_step must be an int, got 2.0"),
    (call_dcnv3, dict(kernel_size=8, stride=65537), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (8, 8)"),
    (call_dcnv3, dict(stride=65537, dilation=65537, padding=65537), ValueError,
     "stride must lie in [1, MAX_DCNV3_STEP = 65536], got (65537, 65537)"),
    (call_dcnv3, dict(input=M(1, 2 ** 24 + 1, 3, 257)), ValueError, "group_channels must lie in [1, MAX_DCNV3_CHANNELS = 256], got 257"),
    (call_dcnv3_function, dict(input=M(3, 3, 2), group=1.0), ValueError, "input must be [N, H, W, C] (channels last), got shape (3, 3, 2)"),
    (call_dcnv3_function, dict(group_channels=2.0, offset_scale="x"), TypeError, "group_channels must be an int, got 2.0"),
    (call_dcnv3_function, dict(group=None, group_channels=None, im2col_step=None), TypeError, "group must be an int, got None"),
    (call_dcnv3_function, dict(im2col_step=0, group=0), ValueError, "im2col_step must be at least 1, got 0"),
    (call_dcnv3_function, dict(group_channels=257, kernel_h=8), ValueError,
     "group * group_channels must equal input's 2 channels, got group 1 and group_channels 257"),
    (call_dcnv3_function, dict(kernel_h=0, input=None), ValueError, "kernel_h, kernel_w must be >= 1, got (0, 3)"),
    (call_dcnv4, dict(remove_center="yes", im2col_step=1.5), TypeError, "im2col_step must be an int, got 1.5"),
    (call_dcnv4, dict(remove_center="yes", offset_scale="1"), TypeError, "remove_center must be a bool, got 'yes'"),
    (call_dcnv4, dict(remove_center=2, offset_scale=float("inf")), ValueError, "remove_center must be False or True (0 or 1), got 2"),
    (call_dcnv4, dict(remove_center=2, kernel_size=(3, 5)), ValueError, "remove_center must be False or True (0 or 1), got 2"),
    (call_dcnv4, dict(remove_center=True, kernel_size=8), ValueError, "kernel_size must lie in [1, MAX_DCNV3_KERNEL = 7], got (8, 8)"),
    (call_dcnv4, dict(remove_center=True, kernel_size=(3, 5), stride=65537), ValueError,
     "remove_center requires a square kernel of odd size >= 3, got (3, 5)"),
    (call_dcnv4, dict(remove_center=True, kernel_size=4, input=M(1, 3, 3, 257)), ValueError,
     "group_channels must lie in [1, MAX_DCNV3_CHANNELS = 256], got 257"),
    (call_dcnv4, dict(offset_mask=M(1, 1, 1, 27), input=M(1, 2 ** 24 + 1, 3, 2)), ValueError,
     "input must have H and W of at most MAX_DCNV3_SIDE = 16777216, got shape (1, 16777217, 3, 2)"),
    (call_dcnv4_function, dict(remove_center=None, group_channels=2.0), TypeError, "group_channels must be an int, got 2.0"),
    (call_dcnv4_function, dict(remove_center=None, im2col_step=0), TypeError, "remove_center must be a bool, got None"),
    (call_dcnv4_function, dict(offset_scale=float("nan"), group=0), ValueError, "offset_scale must be finite, got nan"),
    # multi_scale_deformable_attn
    (call_msda, dict(value=[1]), TypeError, "value must be a torch.Tensor, got list"),
    (call_msda, dict(value=M(1, 4, 1, 2, dtype=F64)), TypeError, "value must be float32, float16 or bfloat16, got torch.float64"),
    (call_msda, dict(value=M(1, 4, 1, 2, device="cpu")), ValueError, "value must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_msda, dict(sampling_locations=None), TypeError, "sampling_locations must be a torch.Tensor, got NoneType"),
    (call_msda, dict(sampling_locations=M(1, 1, 1, 1, 1, 2, dtype=F16)), TypeError, "sampling_locations must be float32, got torch.float16"),
    (call_msda, dict(value=M(1, 4, 1, 2, dtype=F16), sampling_locations=M(1, 1, 1, 1, 1, 2, dtype=BF16)), TypeError,
     "sampling_locations must be float32 or the value's torch.float16, got torch.bfloat16"),
    (call_msda, dict(attention_weights=M(1, 1, 1, 1, 1, dtype=F64)), TypeError, "attention_weights must be float32, got torch.float64"),
    (call_msda, dict(value=M(1, 4, 1, 2, dtype=BF16), attention_weights=M(1, 1, 1, 1, 1, dtype=F16)), TypeError,
     "attention_weights must be float32 or the value's torch.bfloat16, got torch.float16"),
    (call_msda, dict(value_spatial_shapes=M(1, 2, dtype=I32)), TypeError, "value_spatial_shapes must be int64, got torch.int32"),
    (call_msda, dict(value_spatial_shapes=[(2, 2)]), TypeError, "value_spatial_shapes must be a torch.Tensor, got list"),
    (call_msda, dict(value_level_start_index=M(1, dtype=F32)), TypeError, "value_level_start_index must be int64, got torch.float32"),
    (call_msda, dict(value_level_start_index=M(1, dtype=I64, device="cpu")), ValueError,
     "value_level_start_index must be a tensor on the GPU, got device cpu" + NO_CPU),
    (call_msda, dict(value=M(4, 1, 2)), ValueError, "value must be [B, S, M, D], got shape (4, 1, 2)"),
    (call_msda, dict(sampling_locations=M(1, 1, 1, 1, 1, 3)), ValueError,
     "sampling_locations must be [B, Q, M, L, P, 2], got shape (1, 1, 1, 1, 1, 3)"),
    (call_msda, dict(sampling_locations=M(1, 1, 1, 1, 2)), ValueError,
     "sampling_locations must be [B, Q, M, L, P, 2], got shape (1, 1, 1, 1, 2)"),
    (call_msda, dict(sampling_locations=M(2, 1, 1, 1, 1, 2)), ValueError,
     "sampling_locations must be [B, Q, M, L, P, 2] with value's B = 1 and M = 1, got shape (2, 1, 1, 1, 1, 2)"),
    (call_msda, dict(sampling_locations=M(1, 1, 3, 1, 1, 2)), ValueError,
     "sampling_locations must be [B, Q, M, L, P, 2] with value's B = 1 and M = 1, got shape (1, 1, 3, 1, 1, 2)"),
    (call_msda, dict(attention_weights=M(1, 1, 1, 1, 2)), ValueError,
     "attention_weights must be [B, Q, M, L, P] = [1, 1, 1, 1, 1], got shape (1, 1, 1, 1, 2)"),
    (call_msda, dict(value_spatial_shapes=M(2, 2, dtype=I64)), ValueError, "value_spatial_shapes must be [L, 2] = [1, 2], got shape (2, 2)"),
    (call_msda, dict(value_level_start_index=M(2, dtype=I64)), ValueError, "value_level_start_index must be [L] = [1], got shape (2,)"),
    (call_msda, dict(im2col_step=64.0), TypeError, "im2col_step must be an int, got 64.0"),
    (call_msda, dict(im2col_step=True), TypeError, "im2col_step must be an int, got True"),
    (call_msda, dict(im2col_step=0), ValueError, "im2col_step must be at least 1, got 0"),
    (call_msda, LEVELS9, ValueError, "multi_scale_deformable_attn takes at most MAX_MSDA_LEVELS = 8 levels, got 9"),
    (call_msda, dict(sampling_locations=M(1, 1, 1, 1, 17, 2), attention_weights=M(1, 1, 1, 1, 17)), ValueError,
     "multi_scale_deformable_attn takes at most MAX_MSDA_POINTS = 16 points per level, got 17"),
    (call_msda, dict(value=M(1, 4, 1, 257)), ValueError,
     "multi_scale_deformable_attn takes at most MAX_MSDA_CHANNELS = 256 channels per head, got 257"),
    (call_msda, dict(value=M(1, 2 ** 32, 1, 2)), ValueError,
     "multi_scale_deformable_attn is too large for the kernels' 32-bit cell indices: 1 images x S x M = 4294967296 > MAX_MSDA_INDEX = "
     "2147482623" + LOWER),
    (call_msda, dict(sampling_locations=M(1, 2 ** 30, 1, 1, 1, 2), attention_weights=M(1, 2 ** 30, 1, 1, 1)), ValueError,
     "multi_scale_deformable_attn is too large for the kernels' 32-bit plan indices: 1 images x Q x M x L x P x 4 = 4294967296 > "
     "MAX_MSDA_INDEX = 2147482623" + LOWER),
    (call_msda_function, dict(im2col_step=None), TypeError, "im2col_step must be an int, got None"),
    (call_msda_function, dict(value=M(1, 4, 1, 2, dtype=I64)), TypeError, "value must be float32, float16 or bfloat16, got torch.int64"),
    # msda, two rules at once
    (call_msda, dict(im2col_step=0.5, **LEVELS9), TypeError, "im2col_step must be an int, got 0.5"),
    (call_msda, dict(attention_weights=M(1, 1, 1, 1, 2), value_spatial_shapes=M(2, 2, dtype=I64)), ValueError,
     "attention_weights must be [B, Q, M, L, P] = [1, 1, 1, 1, 1], got shape (1, 1, 1, 1, 2)"),
    (call_msda, dict(value=M(4, 1, 2), sampling_locations=M(1, 1, 1, 1, 1, 2, dtype=F64)), TypeError,
     "sampling_locations must be float32, got torch.float64"),
    (call_msda, dict(value=M(1, 4, 1, 257), im2col_step=0), ValueError, "im2col_step must be at least 1, got 0"),
    (call_msda, dict(value=M(1, 2 ** 32, 1, 257)), ValueError,
     "multi_scale_deformable_attn takes at most MAX_MSDA_CHANNELS = 256 channels per head, got 257"),
    (call_msda, dict(value_level_start_index=M(1, dtype=I32), value_spatial_shapes=M(1, 2, dtype=I32)), TypeError,
     "value_spatial_shapes must be int64, got torch.int32"),
    # carafe's integer rules
    (call_carafe, dict(kernel_size=3.0), TypeError, "kernel_size must be an int, got 3.0"),
    (call_carafe, dict(kernel_size=True), TypeError, "kernel_size must be an int, got True"),
    (call_carafe, dict(kernel_size=9), ValueError, "kernel_size must lie in [1, 7] (MAX_CARAFE_KERNEL), got 9"),
    (call_carafe, dict(kernel_size=0), ValueError, "kernel_size must lie in [1, 7] (MAX_CARAFE_KERNEL), got 0"),
    (call_carafe, dict(kernel_size=2), ValueError, "kernel_size must be odd, got 2"),
    (call_carafe, dict(scale_factor=2.0), TypeError, "scale_factor must be an int, got 2.0"),
    (call_carafe, dict(scale_factor=False), TypeError, "scale_factor must be an int, got False"),
    (call_carafe, dict(scale_factor=9), ValueError, "scale_factor must lie in [1, 8] (MAX_CARAFE_SCALE), got 9"),
    (call_carafe, dict(scale_factor=0), ValueError, "scale_factor must lie in [1, 8] (MAX_CARAFE_SCALE), got 0"),
    (call_carafe, dict(group_size=None), TypeError, "group_size must be an int, got None"),
    (call_carafe, dict(group_size=1.0), TypeError, "group_size must be an int, got 1.0"),
    (call_carafe, dict(group_size=0), ValueError, "group_size must lie in [1, 2147483647], got 0"),
    (call_carafe, dict(group_size=2 ** 31), ValueError, "group_size must lie in [1, 2147483647], got 2147483648"),
    (call_carafe, dict(group_size=3), ValueError, "group_size must divide the channels of features, got group_size 3 for 2 channels"),
    (call_carafe, dict(kernel_size=3.0, scale_factor=9), TypeError, "kernel_size must be an int, got 3.0"),
    (call_carafe, dict(scale_factor=0, group_size=1.0), ValueError, "scale_factor must lie in [1, 8] (MAX_CARAFE_SCALE), got 0"),
    (call_carafe, dict(kernel_size=4, scale_factor=2.0), ValueError, "kernel_size must be odd, got 4"),
    # the int-or-pair rule's other callers
    (call_deform_conv2d, dict(stride=1.5), TypeError, "stride must be an int or a pair of ints, got 1.5"),
    (call_deform_conv2d, dict(stride=True), TypeError, "stride must be an int or a pair of ints, got True"),
    (call_deform_conv2d, dict(stride=0), ValueError, "stride must be >= 1, got (0, 0)"),
    (call_deform_conv2d, dict(padding=[1, True]), TypeError, "padding must be an int or a pair of ints, got [1, True]"),
    (call_deform_conv2d, dict(padding=(-1, 0)), ValueError, "padding must be >= 0, got (-1, 0)"),
    (call_deform_conv2d, dict(dilation=(1, 2, 3)), TypeError, "dilation must be an int or a pair of ints, got (1, 2, 3)"),
    (call_deform_conv2d, dict(dilation=(1, 0)), ValueError, "dilation must be >= 1, got (1, 0)"),
    (call_deform_conv2d, dict(stride=0, padding=-1, dilation=0), ValueError, "stride must be >= 1, got (0, 0)"),
    (call_deform_module, dict(kernel_size=0), ValueError, "kernel_size must be >= 1, got (0, 0)"),
    (call_deform_module, dict(kernel_size=3.0), TypeError, "kernel_size must be an int or a pair of ints, got 3.0"),
    (call_deform_module, dict(stride=(1, 1, 1)), TypeError, "stride must be an int or a pair of ints, got (1, 1, 1)"),
    (call_deform_module, dict(padding=-2), ValueError, "padding must be >= 0, got (-2, -2)"),
    (call_deform_module, dict(dilation=[0, 0]), ValueError, "dilation must be >= 1, got (0, 0)"),
]


def _row_id(row):
    return "%s-%s" % (row[0].__name__[5:], "+".join(row[1]))


@pytest.mark.parametrize("row", TABLE, ids=[_row_id(r) + "-%d" % i for i, r in enumerate(TABLE)])
def test_the_error_is_raised_with_its_whole_message(row):
    call, broken, kind, message = row
    with pytest.raises(Exception) as caught:
        call(**broken)
    assert type(caught.value) is kind and str(caught.value) == message


@pytest.mark.parametrize("call", [call_dcnv3, call_dcnv4, call_dcnv3_function, call_dcnv4_function, call_msda, call_msda_function,
                                  call_carafe, call_deform_conv2d])
def test_the_valid_calls_of_the_table_pass_every_rule(call):
    """So each row fails by what it breaks, and by nothing else: on meta tensors the unbroken call runs through to the op's fake result."""
    assert call().device.type == "meta"
