"""float64 restatement of the reference's evaluation metrics (test.py:129-136, :157-175), the checker of sesrq.quality.

skimage is not installed, so its defaults are restated here: structural_similarity with a 7x7 uniform window, K1 = 0.01, K2 = 0.03,
sample covariance (49/48), C1 = (K1 R)^2, C2 = (K2 R)^2, the SSIM map averaged over the windows wholly inside the frame (cropped by 3
pixels on each side); peak_signal_noise_ratio = 10 log10(R^2 / mse).  Frames are (N, C, H, W); the prediction is clipped to [0, 1],
the ground truth is not."""
import numpy as np

WIN = 7
PAD = WIN // 2
Y_WEIGHTS = (65.481, 128.553, 24.966)


def box_mean(a):
    """Mean of every 7x7 window that lies wholly inside the last two axes: (..., H, W) -> (..., H - 6, W - 6), float64."""
    a = np.asarray(a, np.float64)
    c = np.cumsum(a, axis=-1)
    c = np.concatenate([np.zeros(c.shape[:-1] + (1,)), c], axis=-1)
    h = c[..., WIN:] - c[..., :-WIN]
    c = np.cumsum(h, axis=-2)
    c = np.concatenate([np.zeros(c.shape[:-2] + (1,) + c.shape[-1:]), c], axis=-2)
    return (c[..., WIN:, :] - c[..., :-WIN, :]) / (WIN * WIN)


def window_moments(x, y):
    """(ux, uy, vx, vy, vxy) of two (H, W) images over every 7x7 window wholly inside them: the window means and skimage's sample
    (co)variances (49/48), float64, each of shape (H - 6, W - 6)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if x.shape[-1] < WIN or x.shape[-2] < WIN:
        raise ValueError("frame smaller than the 7x7 window")
    ux, uy = box_mean(x), box_mean(y)
    uxx, uyy, uxy = box_mean(x * x), box_mean(y * y), box_mean(x * y)
    cov = WIN * WIN / (WIN * WIN - 1.0)
    return ux, uy, cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)


def ssim_map(x, y, data_range=1.0):
    """The SSIM map skimage averages: one value per 7x7 window wholly inside two (H, W) images, (H - 6, W - 6), float64."""
    ux, uy, vx, vy, vxy = window_moments(x, y)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_channel(x, y, data_range=1.0):
    """skimage structural_similarity of two (H, W) images with its default arguments."""
    return float(ssim_map(x, y, data_range).mean(dtype=np.float64))


def luma255(img):
    """rgb_to_yuv of the reference on a (3, H, W) image: clip(65.481 R + 128.553 G + 24.966 B + 16, 0, 255)."""
    img = np.asarray(img, np.float64)
    y = img[0] * Y_WEIGHTS[0] + img[1] * Y_WEIGHTS[1] + img[2] * Y_WEIGHTS[2] + 16.0
    return np.clip(y, 0.0, 255.0)


def eps_psnr(mse, data_range=255.0, eps=1e-8):
    """compute_psnr of the reference, given its mean squared error."""
    return float(10.0 * np.log10(data_range ** 2 / (mse + eps)))


def frame_metrics(pred, gt, mflag):
    """(mse, psnr, ssim) of one (C, H, W) frame in the form MFLAG uses; mse in the units its PSNR is formed from."""
    p = np.clip(np.asarray(pred, np.float64), 0.0, 1.0)
    g = np.asarray(gt, np.float64)
    if mflag in (3, 4):
        mse = float(np.mean((g - p) ** 2))
        psnr = float("inf") if mse == 0.0 else float(10.0 * np.log10(1.0 / mse))
    elif mflag == 5:
        mse = float(np.mean((g[0] * 255.0 - p[0] * 255.0) ** 2))
        psnr = eps_psnr(mse)
    elif mflag == 6:
        mse = float(np.mean((luma255(g) - luma255(p)) ** 2))
        psnr = eps_psnr(mse)
    else:
        raise ValueError(f"MFLAG {mflag} has no metric here")
    ssim = float(np.mean([ssim_channel(g[c], p[c]) for c in range(g.shape[0])]))
    return mse, psnr, ssim


def metrics(pred, gt, mflag):
    """(N, 3) float64 of (mse, psnr, ssim) per frame of (N, C, H, W) arrays."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape or pred.ndim != 4:
        raise ValueError("pred and gt must be (N, C, H, W) of one shape")
    return np.array([frame_metrics(pred[n], gt[n], mflag) for n in range(pred.shape[0])], np.float64)
