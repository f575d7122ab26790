"""float64 restatement of the reference's MFLAG 1 (nr) metric (test.py:121-127, :157-173), the checker of sesrq.quality's mosaic form.

The reference clips the prediction to [0, 1], takes ``three2one`` of the prediction and of the ground truth -- the H x W Bayer mosaic
whose pixel (r, c) is channel (r & 1) + (c & 1): R where both are even, G where exactly one is odd, B where both are odd -- and scores
the two mosaics with skimage's peak_signal_noise_ratio (data_range 1) and single-channel structural_similarity.  skimage is not
installed, so its defaults are the restatement of tests/quality_oracle.py.  Frames are (N, 3, H, W)."""
import numpy as np

import quality_oracle as Q


def channel_map(H, W):
    """(H, W) int: the channel three2one selects at each pixel."""
    return (np.arange(H)[:, None] & 1) + (np.arange(W)[None, :] & 1)


def three2one(t):
    """The Bayer mosaic of (..., 3, H, W) frames, (..., H, W), in the frames' dtype: a gather, no arithmetic."""
    t = np.asarray(t)
    if t.ndim < 3 or t.shape[-3] != 3:
        raise ValueError("three2one takes (..., 3, H, W) frames")
    idx = np.broadcast_to(channel_map(*t.shape[-2:]), t.shape[:-3] + (1,) + t.shape[-2:])
    return np.take_along_axis(t, idx, axis=-3)[..., 0, :, :]


def selected(H, W):
    """(3, H, W) bool: the (channel, pixel) positions three2one reads."""
    return channel_map(H, W)[None] == np.arange(3)[:, None, None]


def frame_metrics(pred, gt):
    """(mse, psnr, ssim) of one (3, H, W) frame: np.clip(pred), three2one of both, skimage PSNR (data_range 1, +inf at mse == 0) and
    the single-channel SSIM."""
    x = three2one(np.clip(np.asarray(pred, np.float64), 0.0, 1.0))
    y = three2one(np.asarray(gt, np.float64))
    mse = float(np.mean((y - x) ** 2))
    psnr = float("inf") if mse == 0.0 else float(10.0 * np.log10(1.0 / mse))
    return mse, psnr, Q.ssim_channel(y, x)


def metrics(pred, gt):
    """(N, 3) float64 of (mse, psnr, ssim) per frame of (N, 3, H, W) arrays."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape or pred.ndim != 4 or pred.shape[1] != 3:
        raise ValueError("pred and gt must be (N, 3, H, W) of one shape")
    return np.array([frame_metrics(pred[n], gt[n]) for n in range(pred.shape[0])], np.float64)
