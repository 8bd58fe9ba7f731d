"""The packed output block of an in-flight slot (frcnn_output_block_layout, runtime.block_views): layout arithmetic, no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from fasterrcnn_amd import _native as nv
from fasterrcnn_amd import runtime as rt


@pytest.mark.parametrize("max_rois,ncls", [(300, 21), (300, 2), (1, 2), (128, 91), (512, nv.MAX_NUM_CLASSES), (7, 6)])
def test_layout_alignment_and_no_overlap(max_rois, ncls):
    o_counts, o_cnt, o_det, total = nv.output_block_layout(max_rois, ncls)
    nfg = ncls - 1
    assert o_counts == 0
    for off in (o_counts, o_cnt, o_det, total):
        assert off % 16 == 0                       # every region 16-byte aligned (so the float64 rows are 8-byte aligned)
    assert o_det % 8 == 0
    assert o_cnt >= o_counts + 4 * 4               # int32 counts[4]
    assert o_det >= o_cnt + 4 * nfg                # int32 det_cnt[nfg]
    assert total >= o_det + 8 * 5 * max_rois * nfg  # float64 det[nfg][max_rois][5]
    assert total - (o_det + 40 * max_rois * nfg) < 16 and o_det - (o_cnt + 4 * nfg) < 16      # no more padding than alignment asks


def test_layout_rejects_bad_arguments():
    lib = nv.lib()
    off, total = (C.c_size_t * 3)(), C.c_size_t()
    assert lib.frcnn_output_block_layout(0, 21, off, C.byref(total)) == -1
    assert lib.frcnn_output_block_layout(300, 1, off, C.byref(total)) == -1
    assert lib.frcnn_output_block_layout(300, nv.MAX_NUM_CLASSES + 1, off, C.byref(total)) == -1
    assert lib.frcnn_output_block_layout(300, 21, None, C.byref(total)) == -1
    assert lib.frcnn_output_block_layout(300, 21, off, None) == -1


def test_entry_points_validate_without_gpu():
    lib = nv.lib()
    assert lib.frcnn_stream_depend(None, None, None) == -1
    assert lib.frcnn_ctx_submit_stats(None, None, None) == -1
    assert lib.frcnn_streams_share_queue(None, None, None) == -1
    assert lib.frcnn_predict_submit(None, 0, None, None, None, 600, 1000, None, None, None, None, None, None, None, 300, 1, 0.05, 0.3,
                                    1, None, None, None) == -1


@pytest.mark.parametrize("max_rois,ncls", [(300, 21), (5, 3)])
def test_views_have_the_old_shapes_and_dtypes_and_their_own_bytes(max_rois, ncls):
    o_counts, o_cnt, o_det, total = nv.output_block_layout(max_rois, ncls)
    nfg = ncls - 1
    block = torch.zeros((total,), dtype=torch.uint8)
    counts, det_cnt, det = rt.block_views(block, (o_counts, o_cnt, o_det), max_rois, ncls)
    assert counts.shape == (4,) and counts.dtype == torch.int32
    assert det_cnt.shape == (nfg,) and det_cnt.dtype == torch.int32
    assert det.shape == (nfg, max_rois, 5) and det.dtype == torch.float64
    assert counts.data_ptr() == block.data_ptr() + o_counts
    assert det_cnt.data_ptr() == block.data_ptr() + o_cnt
    assert det.data_ptr() == block.data_ptr() + o_det and det.is_contiguous()
    # writes through one view land in its region only
    counts.fill_(-1)
    det_cnt.fill_(-1)
    det.fill_(1.5)
    raw = block.numpy()
    assert (raw[o_counts:o_counts + 16] == 255).all() and (raw[o_cnt:o_cnt + 4 * nfg] == 255).all()
    assert np.array_equal(raw[o_det:o_det + 40 * nfg * max_rois].view(np.float64), np.full(5 * nfg * max_rois, 1.5))
    pad = np.ones(total, dtype=bool)
    for a, n in ((o_counts, 16), (o_cnt, 4 * nfg), (o_det, 40 * nfg * max_rois)):
        pad[a:a + n] = False
    assert (raw[pad] == 0).all()
