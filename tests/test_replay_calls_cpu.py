"""The refusals of the replay calls' Python wrappers (diff_gaussian_rasterization/_C.py) that need no device: aux_maps,
aux_maps_backward, distortion_map, distortion_map_backward, feature_maps, feature_maps_backward, contribution_scores and
camera_backward, each pinned by exception type and full message, and -- where two refusals apply to one call -- by which of
them wins.  Host tensors only; no GPU needed."""
import pytest
import torch

from diff_gaussian_rasterization import _C

NO_CPU = "the MI355X rasterizer needs device tensors (no CPU path)"
BUF = torch.zeros(64, dtype=torch.uint8)          # a host "state buffer"
VEC = torch.zeros((2, 3), dtype=torch.float32)    # a host model tensor with P = 2
MAT = torch.eye(4)
FEAT = torch.zeros((2, 5), dtype=torch.float32)
STATE = (2, 0, 4, 4, BUF, BUF, BUF)               # P, R, H, W and the three buffers
GEOM = (MAT, MAT, 1.0, 1.0, VEC, VEC, 1.0, torch.zeros((2, 4)), None, torch.ones(2, dtype=torch.int32))


def refused(exc, message, fn, *args, **kwargs):
    with pytest.raises(exc) as e:
        fn(*args, **kwargs)
    assert type(e.value) is exc and str(e.value) == message


def camera_backward(means3D, **kwargs):
    return _C.camera_backward(means3D, None, None, None, VEC, None, 1.0, None, False, MAT, MAT, torch.zeros(3), 1.0, 1.0, 4, 4,
                              None, BUF, None, None, None, **kwargs)


def test_unknown_names():
    refused(ValueError, "aux_maps: unknown map 'nope' (expected a subset of ('depth', 'alpha', 'median_depth'))",
            _C.aux_maps, *STATE, maps=("depth", "nope"))
    grads = "('means2D', 'means3D', 'opacity', 'scales', 'rotations', 'cov3D')"
    refused(ValueError, f"aux_maps_backward: unknown gradient 'nope' (expected a subset of {grads})",
            _C.aux_maps_backward, *STATE, *GEOM, want=("means2D", "nope"))
    refused(ValueError, f"distortion_map_backward: unknown gradient 'features' (expected a subset of {grads})",
            _C.distortion_map_backward, *STATE, *GEOM, None, None, want=("features",))
    refused(ValueError, f"feature_maps_backward: unknown gradient 'nope' (expected a subset of {('features',) + _C.AUX_GRADS})",
            _C.feature_maps_backward, *STATE, *GEOM, FEAT, None, want=("nope",))
    refused(ValueError, "camera_backward: unknown gradient 'nope' (expected a subset of ('viewmatrix', 'projmatrix', 'campos'))",
            camera_backward, VEC, want=("campos", "nope"))
    # ... which wins over the depth mapping's refusal only where it is checked first
    refused(ValueError, "distortion: need near = far = 0 (the linear mapping) or 0 < near < far, got (2.0, 1.0)",
            _C.distortion_map_backward, *STATE, *GEOM, None, None, near=2.0, far=1.0, want=("nope",))


def test_host_tensors_have_no_path():
    refused(RuntimeError, NO_CPU, _C.aux_maps, *STATE)
    refused(RuntimeError, NO_CPU, _C.aux_maps, *STATE, maps=())
    refused(RuntimeError, NO_CPU, _C.aux_maps_backward, *STATE, *GEOM)
    refused(RuntimeError, NO_CPU, _C.distortion_map, *STATE)
    refused(RuntimeError, NO_CPU, _C.distortion_map_backward, *STATE, *GEOM, None, None)
    refused(RuntimeError, NO_CPU, _C.feature_maps, *STATE, FEAT)
    refused(RuntimeError, NO_CPU, _C.feature_maps_backward, *STATE, *GEOM, FEAT, None)
    refused(RuntimeError, NO_CPU, _C.contribution_scores, *STATE)
    refused(RuntimeError, "camera_backward: means3D: " + NO_CPU, camera_backward, VEC)
    refused(RuntimeError, "camera_backward: means3D must have dimensions (num_points, 3)", camera_backward, torch.zeros(6))
    # an empty image buffer: the geometry buffer says where
    refused(RuntimeError, NO_CPU, _C.aux_maps, 2, 0, 4, 4, BUF, BUF, torch.zeros(0, dtype=torch.uint8))
    # it wins over what is checked behind it: an upstream of the wrong size, features of the wrong shape, a bad `out`
    refused(RuntimeError, NO_CPU, _C.aux_maps_backward, *STATE, *GEOM, dL_ddepth=torch.zeros(3))
    refused(RuntimeError, NO_CPU, _C.distortion_map_backward, *STATE, *GEOM, torch.zeros(3), None)
    refused(RuntimeError, NO_CPU, _C.feature_maps_backward, *STATE, *GEOM, torch.zeros((3, 5)), None)
    refused(RuntimeError, NO_CPU, _C.contribution_scores, *STATE, out=[1])
    refused(RuntimeError, NO_CPU, _C.contribution_scores, *STATE, accumulate=True)


def test_feature_tensor_refusals():
    def fm(features):
        return _C.feature_maps(*STATE, features)

    refused(ValueError, "feature_maps: features must be a [P, C] tensor with P = 2, got (2,)", fm, torch.zeros(2))
    refused(ValueError, "feature_maps: features must be a [P, C] tensor with P = 2, got (3, 5)", fm, torch.zeros((3, 5)))
    refused(ValueError, "feature_maps: features must be a [P, C] tensor with P = 2, got list", fm, [[0.0] * 5] * 2)
    refused(ValueError, "feature_maps: need 1 <= C <= 512 feature channels, got C = 0", fm, torch.zeros((2, 0)))
    refused(ValueError, "feature_maps: need 1 <= C <= 512 feature channels, got C = 513", fm, torch.zeros((2, 513)))
    refused(ValueError, "feature_maps: features must be float32, got float64", fm, torch.zeros((2, 5), dtype=torch.float64))
    # shape before channel count before dtype
    refused(ValueError, "feature_maps: features must be a [P, C] tensor with P = 2, got (3, 0)", fm,
            torch.zeros((3, 0), dtype=torch.float64))
    refused(ValueError, "feature_maps: need 1 <= C <= 512 feature channels, got C = 513", fm,
            torch.zeros((2, 513), dtype=torch.float16))
    # ... and the helper itself, with a device to hold the features to
    dev = torch.device("cuda", 0)
    refused(ValueError, f"x: features must live on {dev}, got cpu", _C._feature_tensor, FEAT, 2, dev, "x")
    got, channels = _C._feature_tensor(FEAT.t().contiguous().t()[:0], 0, dev, "x")   # P == 0: nothing to be anywhere
    assert channels == 5 and got.is_contiguous() and tuple(got.shape) == (0, 5)


def test_depth_mapping():
    assert _C.depth_mapping(True) == (0.0, 0.0)
    assert _C.depth_mapping(None) == (0.0, 0.0)
    assert _C.depth_mapping((0, 0)) == (0.0, 0.0)
    assert _C.depth_mapping([0.5, "8"]) == (0.5, 8.0)
    for bad in (False, 5, "ab", (1.0,), (1.0, 2.0, 3.0), (None, 1.0), ("x", 1.0)):
        refused(ValueError, f"distortion: expected True or a (near, far) pair, got {bad!r}", _C.depth_mapping, bad)
    for near, far in ((1.0, 0.5), (1.0, 1.0), (0.0, 1.0), (-1.0, 2.0), (0.0, -0.0 + 1e-30), (float("nan"), 1.0)):
        refused(ValueError, f"distortion: need near = far = 0 (the linear mapping) or 0 < near < far, got ({near}, {far})",
                _C.depth_mapping, (near, far))
    # the two map calls check it before anything else
    refused(ValueError, "distortion: need near = far = 0 (the linear mapping) or 0 < near < far, got (2.0, 1.0)",
            _C.distortion_map, *STATE, near=2.0, far=1.0)
    refused(ValueError, "distortion: expected True or a (near, far) pair, got (None, 1.0)",
            _C.distortion_map_backward, *STATE, *GEOM, None, None, near=None, far=1.0)


def test_contribution_scores_refusals():
    empty = (0, 0, 4, 4, BUF, BUF, BUF)
    names = "('sum', 'max', 'count', 'views')"
    refused(ValueError, "contribution_scores: need P >= 0 and H, W >= 1, got P = -1, 4x4", _C.contribution_scores, -1, 0, 4, 4,
            BUF, BUF, BUF, out=[1])
    refused(ValueError, "contribution_scores: need P >= 0 and H, W >= 1, got P = 0, 4x0", _C.contribution_scores, 0, 0, 0, 4,
            BUF, BUF, BUF)
    refused(ValueError, f"contribution_scores: out must be a dict with names among {names}", _C.contribution_scores, *empty,
            out=[1], accumulate=True)
    refused(ValueError, f"contribution_scores: out must be a dict with names among {names}", _C.contribution_scores, *empty,
            out={"sum": None, "mean": None})
    refused(ValueError, "contribution_scores: accumulate needs the buffers to fold into (out=...)", _C.contribution_scores, *empty,
            accumulate=True)
    refused(ValueError, "contribution_scores: sum must be a tensor, got NoneType", _C.contribution_scores, *empty,
            out={"sum": None})
    refused(RuntimeError, "contribution_scores: max must be a device tensor (no CPU path), got cpu", _C.contribution_scores,
            *empty, out={"max": torch.zeros(0)})
    refused(RuntimeError, "contribution_scores: pixel_weight must be a device tensor (no CPU path), got cpu",
            _C.contribution_scores, *empty, pixel_weight=torch.ones(16))
