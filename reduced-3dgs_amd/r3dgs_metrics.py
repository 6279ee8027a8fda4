"""`r3dgs_metrics` -- the evaluation metrics of the reference on the MI355X, fused in HIP (csrc/metrics.hip,
include/r3dgs_metrics.h): what train.py:246-269 (training_report) and render.py + metrics.py:71-86 judge a model by.

    from r3dgs_metrics import psnr, mse          # instead of: from utils.image_utils import psnr, mse
    from r3dgs_metrics import image_metrics      # L1, MSE, both PSNR conventions and SSIM of one view in one pass
    from r3dgs_metrics import evaluate           # a camera set -> a device-resident [V, ROW] table, no host wait per view
    from r3dgs_metrics import to_uint8           # save_image's 8-bit rounding, on the device

image_metrics clamps like train.py:256-257 (clamp=True), can round the render to 8 bits the way render.py's save_image does
before metrics.py reads it back (quantise=True), and takes the ground truth as float [C,H,W] or as the bytes an image decoder
hands over, uint8 [C,H,W] or [H,W,C] (compared as byte / 255, torchvision's to_tensor).  Results are float64 on the device;
the caller decides when to read them.  LPIPS is not covered: its network weights are not part of this repository.
Inputs are device tensors (there is no CPU path); values are deterministic and the calls can be captured in torch.cuda.graph.
"""
import torch

from diff_gaussian_rasterization import _C

__all__ = ["mse", "psnr", "image_metrics", "to_uint8", "evaluate", "FIELDS", "ROW"]

ROW = _C.METRICS_ROW
FIELDS = ("l1", "mse", "mse_c0", "mse_c1", "mse_c2", "mse_c3", "psnr_image", "psnr_channels", "ssim")
assert len(FIELDS) == ROW


def _check_device_tensor(what, name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} is a host tensor; the fused metrics need device tensors (no CPU path)")
    if t.numel() == 0:
        raise ValueError(f"{what}: {name} is empty")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} is not contiguous; the kernels read it in place (call .contiguous() once, outside "
                         "the evaluation loop)")


def _check_pair(what, a, b):
    for name, t in (("img1", a), ("img2", b)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} is {t.dtype}; the fused metrics take float32 only")
    if a.shape != b.shape:
        raise ValueError(f"{what}: shapes differ, {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.dim() < 1:
        raise ValueError(f"{what}: expected at least one dimension (rows = shape[0]), got a 0-d tensor")
    for name, t in (("img1", a), ("img2", b)):
        _check_device_tensor(what, name, t)
    if a.device != b.device:
        raise ValueError(f"{what}: tensors on {a.device} and {b.device}")


def _row_mse(what, img1, img2):
    _check_pair(what, img1, img2)
    rows = img1.shape[0]
    return _C.row_mse(img1, img2, rows).view(rows, 1)


def mse(img1, img2):
    """utils/image_utils.py:14-15: the mean squared error of each img1[i] against img2[i], [shape[0], 1] float32 (the
    double row mean, rounded once)."""
    return _row_mse("mse", img1, img2).to(torch.float32)


def psnr(img1, img2):
    """utils/image_utils.py:17-19: 20 log10(1 / sqrt(mse)) per img1[i], [shape[0], 1] float32, evaluated in double from the
    double row mean and rounded once."""
    m = _row_mse("psnr", img1, img2)
    return (20.0 * torch.log10(1.0 / torch.sqrt(m))).to(torch.float32)


def _check_image(what, image):
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what}: image must be a tensor")
    if image.dtype != torch.float32:
        raise TypeError(f"{what}: image is {image.dtype}; the fused metrics take a float32 image")
    if image.dim() != 3 or not 1 <= image.shape[0] <= 4:
        raise ValueError(f"{what}: expected an image [C,H,W] with 1 <= C <= 4, got {tuple(image.shape)}")


def _gt_layout(what, image, gt):
    """The R3DGS_GT_* layout of gt, from its dtype and shape; types and shapes of the pair are checked first, then where the
    two tensors lie."""
    _check_image(what, image)
    if not isinstance(gt, torch.Tensor):
        raise TypeError(f"{what}: gt must be a tensor")
    C, H, W = image.shape
    if gt.dtype == torch.float32:
        if gt.shape != image.shape:
            raise ValueError(f"{what}: shapes differ, {tuple(image.shape)} vs {tuple(gt.shape)}")
        layout = _C.GT_F32_CHW
    elif gt.dtype == torch.uint8:
        chw, hwc = tuple(gt.shape) == (C, H, W), tuple(gt.shape) == (H, W, C)
        if not (chw or hwc):
            raise ValueError(f"{what}: shapes differ, image {tuple(image.shape)} vs uint8 gt {tuple(gt.shape)} (expected "
                             f"[C,H,W] or [H,W,C])")
        if chw and hwc and gt.numel() > 1:
            raise ValueError(f"{what}: a uint8 gt of shape {tuple(gt.shape)} is ambiguous, [C,H,W] and [H,W,C] at once; pass "
                             "it as float32 [C,H,W] (gt.float().div(255)) to say which")
        layout = _C.GT_U8_CHW if chw else _C.GT_U8_HWC
    else:
        raise TypeError(f"{what}: gt is {gt.dtype}; the fused metrics take a float32 or uint8 ground truth")
    _check_device_tensor(what, "image", image)
    _check_device_tensor(what, "gt", gt)
    if gt.device != image.device:
        raise ValueError(f"{what}: tensors on {image.device} and {gt.device}")
    return layout


def _check_out(what, out, dev):
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (ROW,):
        raise ValueError(f"{what}: out must be a float64 tensor of shape [{ROW}]")
    _check_device_tensor(what, "out", out)
    if out.device != dev:
        raise ValueError(f"{what}: tensors on {dev} and {out.device}")


def _workspace(image):
    C, H, W = image.shape
    return torch.empty((_C.image_metrics_workspace_bytes(C, H, W),), dtype=torch.uint8, device=image.device)


def _flags(clamp, quantise):
    return (_C.METRICS_CLAMP if clamp else 0) | (_C.METRICS_QUANTISE8 if quantise else 0)


def image_metrics(image, gt, *, clamp=True, quantise=False, out=None):
    """L1, MSE, PSNR and SSIM of image [C,H,W] float32 against gt (float32 [C,H,W], uint8 [C,H,W] or uint8 [H,W,C]) in one
    pass -> float64 [ROW] on the device, entries named by FIELDS; with `out` the caller's row is written and returned.
      clamp     both images are clamped to [0, 1] first (train.py:256-257)
      quantise  the image is first rounded to 8 bits the way save_image does (render.py -> PNG -> metrics.py)
    psnr_image is metrics.py's convention (one mean over the image), psnr_channels train.py's (mean of the per-channel
    PSNR)."""
    what = "image_metrics"
    layout = _gt_layout(what, image, gt)
    if out is None:
        out = torch.empty((ROW,), dtype=torch.float64, device=image.device)
    else:
        _check_out(what, out, image.device)
    return _C.image_metrics(image, gt, layout, _flags(clamp, quantise), out, _workspace(image))


def to_uint8(image):
    """save_image's conversion, mul(255).add_(0.5).clamp_(0, 255).to(uint8), of image [C,H,W] float32 -> uint8 [H,W,C]."""
    _check_image("to_uint8", image)
    _check_device_tensor("to_uint8", "image", image)
    return _C.image_to_uint8(image)


def evaluate(cameras, model, pipe, background, *, quantise=False, render=None):
    """The metrics of every camera of `cameras` for `model` (a GaussianModel-shaped object or a
    r3dgs_quantised.QuantisedModel): each view is rendered under torch.no_grad() with r3dgs_render.render (or `render`, same
    signature), clamped like train.py:256-257 (quantise=True: rounded to 8 bits like render.py's PNG as well) and compared
    with camera.original_image where it lies (float32 [C,H,W], uint8 [C,H,W] or uint8 [H,W,C], on the device).
    -> {"per_view": float64 [V, ROW] on the device, "mean": per_view.mean(0), "fields": FIELDS}
    Nothing in the loop waits for the device; the caller decides when to read."""
    what = "evaluate"
    if render is None:
        from r3dgs_render import render
    cameras = list(cameras)
    if not cameras:
        raise ValueError(f"{what}: no cameras")
    if not isinstance(background, torch.Tensor) or not background.is_cuda:
        raise RuntimeError(f"{what}: background is a host tensor; the fused metrics need device tensors (no CPU path)")
    table = torch.empty((len(cameras), ROW), dtype=torch.float64, device=background.device)
    flags = _flags(True, quantise)
    workspace = None
    with torch.no_grad():
        for v, camera in enumerate(cameras):
            image = render(camera, model, pipe, background)["render"]
            layout = _gt_layout(what, image, camera.original_image)
            if workspace is None or workspace.shape_key != tuple(image.shape):
                workspace = _Workspace(image)
            _C.image_metrics(image, camera.original_image, layout, flags, table[v], workspace.bytes)
    return {"per_view": table, "mean": table.mean(0), "fields": FIELDS}


class _Workspace:
    """The scratch of one image shape, reused from view to view (the launches of a view follow the previous view's on the
    same stream)."""
    __slots__ = ("shape_key", "bytes")

    def __init__(self, image):
        self.shape_key = tuple(image.shape)
        self.bytes = _workspace(image)
