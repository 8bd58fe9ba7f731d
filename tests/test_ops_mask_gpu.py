"""fasterrcnn_amd.ops.paste_masks_in_image / paste_masks_aligned / masks_to_boxes on the GPU against the float64 truths of
tests/mask_cases.py (the contracts of include/frcnn_hip.h in float64, the integer boxes from the float32 sequence).

Bounds are derived, not measured (tests/mask_cases.py): a pasted float32 value lies within tol_k = (10 (M' + 1) + 8) 2^-24 max|mask_k| of
the truth; a threshold decision is compared where the truth is farther than tol_k from the threshold (at most 0.1 % of the non-zero-truth
pixels may be nearer), a uint8 value where 255 truth is farther than 255 tol_k from an integer (at most 3 % may be nearer; within 1
there).  The exact cases, the supports, the 16-bit identities, masks_to_boxes and the run-to-run comparisons are equalities.

Every test prints the figure it asserts on.  Measured on an MI355X: the largest |got - truth| / tol_k is 0.096; the exact cases, the
supports and the 16-bit identities hold without a differing element; no threshold decision and no uint8 value is wrong outside the
left-out pixels, which are at most 5 of 35314 non-zero-truth pixels for bool ("pieces" at 0.5) and at most 1.8 % for uint8 (4 of 228 on
"a_max", which the 3 % bound does not cover; 0.98 % on "pieces", 0.84 % on "a28" among the cases it does); the largest uint8 difference
on a left-out pixel is 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import ops

from tests import mask_cases as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
IDS = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16", torch.bool: "bool", torch.uint8: "u8"}
half = pytest.mark.parametrize("dtype", M.HALF, ids=("f16", "bf16"))
ELEM = {torch.float32: nv.OPS_F32, torch.float16: nv.OPS_F16, torch.bfloat16: nv.OPS_BF16}


@functools.lru_cache(maxsize=None)
def in_image_gpu(name, dtype=F32):
    masks, boxes, shape, p = M.in_image_case(name, dtype)
    return masks.to(DEV), boxes.to(DEV), shape, p


@functools.lru_cache(maxsize=None)
def aligned_gpu(name, dtype=F32):
    masks, boxes, shape = M.aligned_case(name, dtype)
    return masks.to(DEV), boxes.to(DEV), shape


def bits(t):
    return t.view(torch.int16) if t.dtype in M.HALF else t.view(torch.int32)


def plus_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. paste_masks_in_image -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.IN_IMAGE)
def test_in_image_values_against_the_truth(name):
    """Largest |got - truth| / tol_k measured on an MI355X: 0.096 ("m28"; 0.020 at the largest M, "m_max"; 0.092 on "pieces")."""
    masks, boxes, shape, p = in_image_gpu(name)
    got = ops.paste_masks_in_image(masks, boxes, shape, p)
    assert got.shape == (len(boxes), 1) + shape and got.dtype == F32 and got.is_contiguous()
    got = got[:, 0].cpu()
    want = M.in_image_truth(name)
    tol = M.tolerance(masks.cpu(), masks.shape[2] + 2 * p)[:, None, None]
    ratio = float(((got.double() - want).abs() / tol).max())
    print("%s largest |got - truth| / tol_k %.4f" % (name, ratio))
    assert ratio <= 1
    outside = torch.ones_like(got, dtype=torch.bool)
    for k, s in enumerate(M.support_in_image(boxes.cpu(), masks.shape[2], p, shape)):
        if s is not None:
            outside[k, s[1]:s[3] + 1, s[0]:s[2] + 1] = False
    assert plus_zero(got[outside])                                             # +0.0 exactly outside the integer box


def test_in_image_exact_cases():
    """M = 14, padding 1, mask values multiples of 2^-8, integer sizes 8 .. 64: every coordinate, weight and product is exact in float32."""
    masks, boxes, shape, p = M.exact_case()
    got = ops.paste_masks_in_image(masks.to(DEV), boxes.to(DEV), shape, p)[:, 0].cpu()
    want = M.truth_in_image(masks, boxes, shape, p)
    print("exact: differing pixels %d" % int((got.double() != want).sum()))
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("name", M.SEAMS)
def test_in_image_support_is_the_integer_box(name):
    masks, boxes, shape, p = M.seam_case(name)
    got = ops.paste_masks_in_image(masks.to(DEV), boxes.to(DEV), shape, p)[:, 0].cpu()
    want = M.support_in_image(boxes, masks.shape[2], p, shape)
    have = [M.support_of(g) for g in got]
    print(name, have)
    assert have == want
    assert plus_zero(got[[s is None for s in want]])
    tol = M.tolerance(masks, masks.shape[2] + 2 * p)[:, None, None]
    assert bool(((got.double() - M.truth_in_image(masks, boxes, shape, p)).abs() <= tol).all())


@pytest.mark.parametrize("kind", ("X0", "X1", "Y0", "Y1"))
def test_in_image_no_fused_multiply_add_in_the_integer_box(kind):
    """Boxes on which x_c -+ w_half * s lands on another integer when the product is not rounded (tests/mask_cases.py finds them)."""
    boxes = M.fma_boxes()[kind]
    masks = torch.ones((len(boxes), 1, M.FMA_M, M.FMA_M))
    got = ops.paste_masks_in_image(masks.to(DEV), boxes.to(DEV), M.SEAM_SHAPE, M.FMA_P)[:, 0].cpu()
    want = M.support_in_image(boxes, M.FMA_M, M.FMA_P, M.SEAM_SHAPE)
    have = [M.support_of(g) for g in got]
    print(kind, have, want)
    assert have == want


@half
@pytest.mark.parametrize("name", ("m7", "m28", "m28_p2", "m_max", "pieces"))
def test_in_image_16_bit_is_the_float32_operator_rounded_once(name, dtype):
    masks, boxes, shape, p = in_image_gpu(name, dtype)
    got = ops.paste_masks_in_image(masks, boxes, shape, p)
    wide = ops.paste_masks_in_image(masks.float(), boxes, shape, p).to(dtype)
    assert got.dtype == dtype
    print("%s %s differing elements %d" % (name, IDS[dtype], int((bits(got) != bits(wide)).sum())))
    assert torch.equal(bits(got), bits(wide))


# ---- 2. paste_masks_aligned --------------------------------------------------------------------------------------------------------------
def check_bool(label, got, truth, dead, tol, thr):
    thr32 = float(np.float32(thr))
    far = (truth - thr32).abs() > tol
    want = (truth >= thr32) & ~dead
    nonzero = int((truth != 0).sum())
    left_out = int((~far & (truth != 0)).sum())
    wrong = int((got != want)[far].sum())
    print("%s threshold %g: wrong %d, left out %d of %d non-zero-truth pixels" % (label, thr, wrong, left_out, nonzero))
    assert wrong == 0 and left_out <= 0.001 * nonzero
    zero = (truth == 0) & ~dead                                                # a live row's value is >= 0 on these masks: 0 >= threshold
    assert torch.equal(got[zero], torch.full_like(got[zero], 0.0 >= thr32))
    assert not bool(got[dead.expand_as(got)].any())


def check_uint8(label, got, truth, dead, tol, share):
    q = truth * 255
    want = q.trunc().clamp(0, 255)
    far = (q - q.round()).abs() > 255 * tol
    nonzero = int((truth != 0).sum())
    left_out = int((~far & (truth != 0)).sum())
    diff = (got.double() - want).abs()
    print("%s uint8: wrong %d, largest difference %g, left out %d of %d non-zero-truth pixels" % (label, int((diff[far] != 0).sum()), float(diff.max()),
                                                                                                   left_out, nonzero))
    assert not bool((diff[far] != 0).any()) and float(diff.max()) <= 1
    if share is not None:
        assert left_out <= share * nonzero
    assert not bool(got[dead.expand_as(got)].any())


@pytest.mark.parametrize("name", tuple(M.ALIGNED) + ("seams",))
def test_aligned_bool_and_uint8_against_the_truth(name):
    masks, boxes, shape = aligned_gpu(name)
    truth = M.aligned_truth(name)
    dead = torch.from_numpy(M.dead_aligned(boxes.cpu()))[:, None, None]
    tol = M.tolerance(masks.cpu(), max(masks.shape[1:]))[:, None, None]
    for thr in M.THRESHOLDS:
        got = ops.paste_masks_aligned(masks, boxes, shape, thr)
        assert got.dtype == torch.bool and got.shape == truth.shape and got.is_contiguous()
        assert int(got.view(torch.uint8).max()) <= 1
        check_bool(name, got.cpu(), truth, dead, tol, thr)
    got = ops.paste_masks_aligned(masks, boxes, shape, -1.0)
    assert got.dtype == torch.uint8 and got.shape == truth.shape
    check_uint8(name, got.cpu(), truth, dead, tol, 0.03 if name in M.UINT8_CASES else None)
    assert torch.equal(ops.paste_masks_aligned(masks[:, None], boxes, shape, 0.5), ops.paste_masks_aligned(masks, boxes, shape, 0.5))
    assert torch.equal(ops.paste_masks_aligned(masks[:, None], boxes, shape, -1.0), got)


def test_aligned_seams_dead_rows_are_false_at_every_threshold():
    masks, boxes, shape = aligned_gpu("seams")
    dead = torch.from_numpy(M.dead_aligned(boxes.cpu()))
    got = ops.paste_masks_aligned(masks, boxes, shape, 0.0).cpu()
    assert not bool(got[dead].any()) and bool(got[~dead].all())
    assert not bool(ops.paste_masks_aligned(masks, boxes, shape, -1.0).cpu()[dead].any())


@half
@pytest.mark.parametrize("name", ("a7", "a28", "a7x14", "a_max", "pieces", "seams"))
def test_aligned_16_bit_equals_the_float32_operator_on_the_widened_masks(name, dtype):
    masks, boxes, shape = aligned_gpu(name, dtype)
    for thr in (0.5, -1.0):
        assert torch.equal(ops.paste_masks_aligned(masks, boxes, shape, thr), ops.paste_masks_aligned(masks.float(), boxes, shape, thr))


# ---- 3. masks_to_boxes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.BOX_DTYPES, ids=[IDS[d] for d in M.BOX_DTYPES])
@pytest.mark.parametrize("name", M.BOXES_CASES)
def test_masks_to_boxes_equals_the_twin(name, dtype):
    masks = M.boxes_case(name, dtype)
    got = ops.masks_to_boxes(masks.to(DEV))
    assert got.dtype == F32 and got.shape == (masks.shape[0], 4)
    assert torch.equal(got.cpu(), ops.masks_to_boxes_pytorch(masks)) and torch.equal(got.cpu(), M.boxes_truth(masks))


@pytest.mark.parametrize("dtype", M.DTYPES, ids=[IDS[d] for d in M.DTYPES])
def test_masks_to_boxes_nan_minus_zero_views_and_empty(dtype):
    m = torch.zeros((5, 33, 47), dtype=dtype)
    m[0, 4, 6] = float("nan")
    m[1, 2, 3] = -0.0
    m[3, 32, 46] = -1.0
    m[4, 0, 0] = float("nan")
    m[4, 20, 30] = -0.0
    want = torch.tensor([[6.0, 4, 6, 4], [0, 0, 0, 0], [0, 0, 0, 0], [46, 32, 46, 32], [0, 0, 0, 0]])
    g = m.to(DEV)
    assert torch.equal(ops.masks_to_boxes(g).cpu(), want) and torch.equal(ops.masks_to_boxes_pytorch(m), want)
    for view in (g.transpose(1, 2), g[::2], g[:, 1:30:2, 3:40], g.expand(5, 33, 47)[:, :, ::3]):             # non-contiguous views
        assert not view.is_contiguous()
        assert torch.equal(ops.masks_to_boxes(view).cpu(), ops.masks_to_boxes_pytorch(view.cpu()))
    assert ops.masks_to_boxes(g[:0]).shape == (0, 4)
    one = torch.zeros((1, 1, 1), dtype=dtype, device=DEV)
    assert torch.equal(ops.masks_to_boxes(one + 1).cpu(), torch.zeros(1, 4))                                 # the pixel (0, 0)


# ---- 4. all three: two runs, a poisoned output, graph capture, K = 0 -----------------------------------------------------------------------
def calls():
    masks, boxes, shape, p = in_image_gpu("pieces")
    am, ab, ashape = aligned_gpu("a7x14")
    bm = M.boxes_case("pieces", torch.float16).to(DEV)
    return {"in_image": lambda: ops.paste_masks_in_image(masks, boxes, shape, p),
            "in_image_bf16": lambda: ops.paste_masks_in_image(in_image_gpu("m28", torch.bfloat16)[0], *in_image_gpu("m28", torch.bfloat16)[1:]),
            "aligned_bool": lambda: ops.paste_masks_aligned(am, ab, ashape, 0.5),
            "aligned_uint8": lambda: ops.paste_masks_aligned(am, ab, ashape, -1.0),
            "masks_to_boxes": lambda: ops.masks_to_boxes(bm)}


CALLS = ("in_image", "in_image_bf16", "aligned_bool", "aligned_uint8", "masks_to_boxes")


@pytest.mark.parametrize("which", CALLS)
def test_two_runs_agree_bit_for_bit(which):
    f = calls()[which]
    a, b = f(), f()
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("which", CALLS)
def test_graph_capture_succeeds(which):
    """Nothing synchronises with the host: the call is legal inside a stream capture, and the replay gives the eager result."""
    f = calls()[which]
    eager = f()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = f()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.uint8), eager.view(torch.uint8))


@pytest.mark.parametrize("dtype", M.DTYPES, ids=[IDS[d] for d in M.DTYPES])
@pytest.mark.parametrize("shift", (0, 1, 3))
def test_in_image_writes_every_element_of_a_poisoned_output(dtype, shift):
    """The output starts as 0xFF bytes (NaNs) and begins `shift` elements into its buffer, so that heads and tails differ."""
    masks, boxes, shape, p = in_image_gpu("m28", dtype)
    k, hw = len(boxes), shape[0] * shape[1]
    want = ops.paste_masks_in_image(masks, boxes, shape, p)
    buf = torch.full(((k * hw + shift + 8) * masks.element_size(),), 0xFF, dtype=torch.uint8, device=DEV).view(dtype)
    rc = nv.lib().frcnn_ops_paste_masks_in_image(ELEM[dtype], masks.data_ptr(), boxes.data_ptr(), k, masks.shape[2], p, shape[0], shape[1],
                                                 buf.data_ptr() + shift * masks.element_size(), stream())
    assert rc == 0
    assert torch.equal(bits(buf[shift:shift + k * hw].contiguous()), bits(want.reshape(-1)))
    rest = torch.cat([buf[:shift], buf[shift + k * hw:]]).view(torch.uint8)
    assert bool((rest == 0xFF).all())                                          # and nothing beside it


@pytest.mark.parametrize("shift", (0, 5))
@pytest.mark.parametrize("threshold", (0.5, -1.0))
def test_aligned_writes_every_element_of_a_poisoned_output(threshold, shift):
    masks, boxes, shape = aligned_gpu("a7x14")
    k, hw = len(boxes), shape[0] * shape[1]
    want = ops.paste_masks_aligned(masks, boxes, shape, threshold).view(torch.uint8)
    buf = torch.full((k * hw + shift + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    rc = nv.lib().frcnn_ops_paste_masks_aligned(nv.OPS_F32, masks.data_ptr(), boxes.data_ptr(), k, masks.shape[1], masks.shape[2], shape[0], shape[1],
                                                threshold, int(threshold < 0), buf.data_ptr() + shift, stream())
    assert rc == 0
    assert int(want.max()) < 0xFF                                             # the masks lie in [0, 1): no legal byte is the poison
    assert torch.equal(buf[shift:shift + k * hw], want.reshape(-1))
    assert bool((torch.cat([buf[:shift], buf[shift + k * hw:]]) == 0xFF).all())


def test_masks_to_boxes_needs_no_initial_value_in_output_or_workspace():
    masks = M.boxes_case("pieces", torch.bool).to(DEV)
    n, h, w = masks.shape
    lib = nv.lib()
    ws = torch.full((lib.frcnn_ops_masks_to_boxes_workspace_bytes(n, h, w, 1),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((n * 16,), 0xFF, dtype=torch.uint8, device=DEV).view(F32).view(n, 4)
    assert lib.frcnn_ops_masks_to_boxes(1, masks.data_ptr(), n, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), stream()) == 0
    assert torch.equal(out.cpu(), M.boxes_truth(masks.cpu()))


def test_k_zero():
    e = torch.zeros((0, 1, 7, 7), device=DEV)
    out = ops.paste_masks_in_image(e, torch.zeros((0, 4), device=DEV), (5, 6))
    assert out.shape == (0, 1, 5, 6) and out.dtype == F32
    out = ops.paste_masks_aligned(e, torch.zeros((0, 4), device=DEV), (5, 6))
    assert out.shape == (0, 5, 6) and out.dtype == torch.bool
    assert ops.paste_masks_aligned(e[:, 0].half(), torch.zeros((0, 4), device=DEV), (5, 6), -1.0).dtype == torch.uint8
    assert ops.masks_to_boxes(torch.zeros((0, 5, 6), dtype=torch.bool, device=DEV)).shape == (0, 4)
