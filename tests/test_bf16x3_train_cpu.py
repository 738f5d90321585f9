"""CPU: bf16x3 training (compute_dtype="bf16x3") as the C ABI and the Python surface see it without a GPU -- the new entry points
in the header and the binding, their host-side argument / shape checks (which return before anything is launched), and the
engine / model selection."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(256)          # never dereferenced: every call below returns from its host-side checks
NEW = ("creid_conv2d_dgrad_x3_nhwc", "creid_conv2d_wgrad_x3_workspace_bytes", "creid_conv2d_wgrad_x3_nhwc",
       "creid_conv2d_wgrad_x3_partials", "creid_weight_prep_x3_train_multi")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from centroids_reid_amd import _lib
    _lib.lib()
    return _lib


def test_new_symbols_in_header_and_binding(L):
    txt = open(os.path.join(ROOT, "include", "creid.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in L.SIGNATURES, name
        assert hasattr(L.lib(), name), name
    assert "bf16x3" in L.TRAIN_PRECISIONS


def test_dgrad_x3_host_checks(L):
    lib = L.lib()
    d = L.ConvDesc(2, 8, 8, 64, 8, 8, 128, 3, 3, 1, 1)
    assert lib.creid_conv2d_dgrad_x3_nhwc(C.byref(d), None, FAKE, FAKE, None, None) == -1
    assert lib.creid_conv2d_dgrad_x3_nhwc(C.byref(d), FAKE, None, FAKE, None, None) == -1
    assert lib.creid_conv2d_dgrad_x3_nhwc(C.byref(d), FAKE, FAKE, None, None, None) == -1
    assert lib.creid_conv2d_dgrad_x3_nhwc(None, FAKE, FAKE, FAKE, None, None) == -1
    for bad in (L.ConvDesc(2, 8, 8, 48, 8, 8, 64, 3, 3, 1, 1),      # in_c not a power of two
                L.ConvDesc(2, 8, 8, 64, 8, 8, 32, 3, 3, 1, 1),      # out_c < 64
                L.ConvDesc(2, 8, 8, 64, 8, 8, 64, 5, 5, 1, 2),      # 5 x 5
                L.ConvDesc(2, 8, 8, 64, 4, 4, 64, 3, 3, 3, 1),      # stride 3
                L.ConvDesc(2, 8, 8, 64, 7, 8, 64, 3, 3, 1, 1)):     # inconsistent out_h
        assert lib.creid_conv2d_dgrad_x3_nhwc(C.byref(bad), FAKE, FAKE, FAKE, None, None) == -4


def test_wgrad_x3_host_checks(L):
    lib = L.lib()
    d = L.ConvDesc(2, 8, 8, 64, 8, 8, 128, 3, 3, 1, 1)
    n = lib.creid_conv2d_wgrad_x3_workspace_bytes(C.byref(d))
    assert n > 0 and n == lib.creid_conv2d_wgrad_workspace_bytes(C.byref(d), L.F32)   # the fp32 layout and split count
    assert lib.creid_conv2d_wgrad_x3_workspace_bytes(None) == 0
    bad = L.ConvDesc(2, 8, 8, 48, 8, 8, 64, 3, 3, 1, 1)
    assert lib.creid_conv2d_wgrad_x3_workspace_bytes(C.byref(bad)) == 0
    assert lib.creid_conv2d_wgrad_x3_nhwc(C.byref(d), None, FAKE, FAKE, 0, FAKE, n, None) == -1
    assert lib.creid_conv2d_wgrad_x3_nhwc(C.byref(d), FAKE, FAKE, None, 0, FAKE, n, None) == -1
    assert lib.creid_conv2d_wgrad_x3_nhwc(C.byref(d), FAKE, FAKE, FAKE, 0, None, n, None) == -1
    assert lib.creid_conv2d_wgrad_x3_partials(C.byref(d), FAKE, None, FAKE, n, None) == -1
    assert lib.creid_conv2d_wgrad_x3_partials(None, FAKE, FAKE, FAKE, n, None) == -1
    assert lib.creid_conv2d_wgrad_x3_nhwc(C.byref(bad), FAKE, FAKE, FAKE, 0, FAKE, n, None) == -4
    assert lib.creid_conv2d_wgrad_x3_partials(C.byref(bad), FAKE, FAKE, FAKE, n, None) == -4
    assert lib.creid_conv2d_wgrad_x3_nhwc(C.byref(d), FAKE, FAKE, FAKE, 0, FAKE, n - 4, None) == -3
    assert lib.creid_conv2d_wgrad_x3_partials(C.byref(d), FAKE, FAKE, FAKE, n - 4, None) == -3


def test_weight_prep_x3_train_host_checks(L):
    lib = L.lib()
    assert lib.creid_weight_prep_x3_train_multi(None, FAKE, 1, 1, None) == -1
    assert lib.creid_weight_prep_x3_train_multi(FAKE, None, 1, 1, None) == -1
    assert lib.creid_weight_prep_x3_train_multi(FAKE, FAKE, 0, 1, None) == -1
    assert lib.creid_weight_prep_x3_train_multi(FAKE, FAKE, 1, 0, None) == -1


def _cfg(name="resnet50"):
    from centroids_reid_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.PRETRAINED = False
    cfg.MODEL.NAME = name
    return cfg


def test_trainable_engine_selection():
    from centroids_reid_amd import baseline
    b = baseline.Baseline(_cfg(), compute_dtype="bf16x3")
    e = b.engine_for(True)
    assert e.x3 and e.x3_train and e.dtype == torch.float32 and e.conv_dt == 3
    assert not (e.sched.wred_piggyback or e.sched.fuse_bn_reduce or e.sched.relu_bitmask)    # (no side-stream forms any more)
    assert b.engine_for(True) is e and b.engine is e            # built once, not on every access
    assert b.engine_for(False) is e                             # its eval-mode forward is the folded bf16x3 one
    b2 = baseline.Baseline(_cfg(), compute_dtype="bf16x3", eval_precision="bf16x3")
    assert b2.engine_for(False) is b2.engine_for(True)
    with pytest.raises(ValueError):
        baseline.Baseline(_cfg(), compute_dtype="tf32")


def test_default_x3_engine_stays_eval_only():
    from centroids_reid_amd import _lib, backbone as bb
    net = bb.ResNet(last_stride=1)
    eng = bb.BackboneEngine(net, "bf16x3")
    assert eng.x3 and not eng.x3_train and eng.sched.eval_fold    # (its training forward still raises: tests/test_bf16x3_train_gpu.py)
    with pytest.raises(ValueError):
        bb.BackboneEngine(net, torch.float32, trainable=True)
    # the trainable form refuses the BasicBlock networks with a clear error
    with pytest.raises(_lib.CreidError, match="Bottleneck"):
        bb.BackboneEngine(bb.build_backbone("resnet18", 1), "bf16x3", trainable=True)


def test_eval_precision_on_a_bf16_model_is_unchanged():
    from centroids_reid_amd import baseline
    b = baseline.Baseline(_cfg(), compute_dtype=torch.bfloat16, eval_precision="bf16x3")
    assert b.engine_for(True).dtype == torch.bfloat16 and b.engine_for(True).mode is None
    ev = b.engine_for(False)
    assert ev.x3 and not ev.x3_train and ev is not b.engine_for(True)
    assert b.engine_for(False) is ev


def test_ctl_model_takes_the_mode():
    from centroids_reid_amd.train_ctl_model import CTLModel
    m = CTLModel(_cfg(), num_classes=10, num_query=0, compute_dtype="bf16x3")
    assert m.backbone.compute_dtype == "bf16x3"
    assert m.backbone.engine_for(True).x3_train
    sd = m.state_dict()
    m32 = CTLModel(_cfg(), num_classes=10, num_query=0, compute_dtype=torch.float32)
    assert set(sd) == set(m32.state_dict())                    # checkpoints are interchangeable
    m32.load_state_dict(sd)
