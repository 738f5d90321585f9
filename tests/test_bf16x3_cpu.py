"""CPU: the bf16x3 compute mode (CREID_BF16X3) as the C ABI and the Python surface see it without a GPU -- the enum value,
the ctypes constant, and the host-side argument checks that return before anything is launched."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns from its host-side checks


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import _lib
    _lib.lib()
    return _lib


def test_enum_value_in_header_and_binding(L):
    txt = open(os.path.join(ROOT, "include", "creid.h")).read()
    m = re.search(r"enum\s*\{\s*CREID_F32\s*=\s*0\s*,\s*CREID_BF16\s*=\s*1\s*,\s*CREID_F16\s*=\s*2\s*,\s*CREID_BF16X3\s*=\s*(\d+)\s*\}", txt)
    assert m and int(m.group(1)) == 3
    assert L.BF16X3 == 3 and "bf16x3" in L.EVAL_PRECISIONS
    assert L.BF16X3 not in L._DT.values()          # a convolution mode, not a storage dtype


def test_weight_prep_refuses_a_dgrad_copy(L):
    """bf16x3 is forward-only: asking for the [I][r][s][O] data-gradient copy is an argument error."""
    assert L.lib().creid_weight_prep(FAKE, 64, 64, 3, 3, L.BF16X3, FAKE, FAKE, None) == -1


def test_training_entry_points_refuse_the_mode(L):
    d = L.ConvDesc(2, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1)
    lib = L.lib()
    assert lib.creid_conv2d_dgrad_nhwc(C.byref(d), FAKE, FAKE, FAKE, None, L.BF16X3, None) == -2
    assert lib.creid_conv2d_dgrad_fused_nhwc(C.byref(d), FAKE, FAKE, FAKE, None, 1, None, None, None, None, None, None, None, 0,
                                            None, None, 0, None, 0, L.BF16X3, None) == -2
    assert lib.creid_conv2d_wgrad_reduce_job(C.byref(d), FAKE, 0, FAKE, 1 << 20, L.BF16X3, None) == -2


def test_forward_convolutions_keep_the_shape_checks(L):
    bad = L.ConvDesc(2, 8, 8, 48, 8, 8, 64, 3, 3, 1, 1)          # in_c not a power of two
    lib = L.lib()
    assert lib.creid_conv2d_fwd_nhwc(C.byref(bad), FAKE, FAKE, FAKE, None, L.BF16X3, None) == -4
    assert lib.creid_conv2d_fwd_affine_nhwc(C.byref(bad), FAKE, FAKE, FAKE, FAKE, None, 1, L.BF16X3, None) == -4


def test_engine_mode_and_baseline_argument():
    from centroids_reid_amd import backbone as bb, baseline
    from centroids_reid_amd.config import get_cfg_defaults
    net = bb.ResNet(last_stride=1)
    eng = bb.BackboneEngine(net, "bf16x3")
    assert eng.x3 and eng.dtype == torch.float32 and eng.conv_dt == 3 and eng.sched.eval_fold
    assert not eng.sched.stem_pool_fused or eng.dtype == torch.float32        # the 16-bit-only fused stem is never taken
    with pytest.raises(ValueError):
        bb.BackboneEngine(net, "tf32")
    # engines of one network share the weight-change flag
    eng16 = bb.BackboneEngine(net, torch.bfloat16)
    eng.weights_dirty = False
    eng16.weights_dirty = True
    assert eng.weights_dirty
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    with pytest.raises(ValueError):
        baseline.Baseline(cfg, eval_precision="fp8")
    b = baseline.Baseline(cfg, compute_dtype=torch.bfloat16, eval_precision="bf16x3")
    assert b.engine_for(True).dtype == torch.bfloat16
    assert b.engine_for(False).x3 and b.engine_for(False).dtype == torch.float32
    assert baseline.Baseline(cfg, compute_dtype=torch.bfloat16).engine_for(False).dtype == torch.bfloat16
