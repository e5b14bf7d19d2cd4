"""numpy restatement of the camera front end (include/mof.h, mof_frontend_*): cv::resize by an exact integer factor s on 8-bit
data in its closed forms, the crop, CV_RGB2GRAY as the node applies it to BGR8 data [published OpenCV algorithm, unpinned].
tests/test_frontend_host.py anchors it to the oracle (s = 4 mono: oracle_resize_quarter_u8; s = 1 BGR: oracle_rgb2gray_u8)."""
import numpy as np


def frontend(frames: np.ndarray, s: int, crop=None) -> np.ndarray:
    """frames: uint8 [n, H, W] or [n, H, W, 3]; crop = (x, y, width, height) in the downscaled image (None: all of it)
    -> uint8 [n, height, width]."""
    f = np.asarray(frames).astype(np.uint32)
    h, w = f.shape[1] // s, f.shape[2] // s
    x0, y0, cw, ch = crop if crop is not None else (0, 0, w, h)
    off = (s - 1) // 2  # odd s: the single tap; even s: the first of the two taps
    rows, cols = s * (y0 + np.arange(ch)) + off, s * (x0 + np.arange(cw)) + off
    if s % 2:
        r = f[:, rows][:, :, cols]
    else:
        r = (f[:, rows][:, :, cols] + f[:, rows][:, :, cols + 1] + f[:, rows + 1][:, :, cols] + f[:, rows + 1][:, :, cols + 1] + 2) >> 2
    if r.ndim == 4:  # byte 0 gets the R weight (CV_RGB2GRAY on BGR data)
        r = (r[..., 0] * 4899 + r[..., 1] * 9617 + r[..., 2] * 1868 + 8192) >> 14
    return np.ascontiguousarray(r, dtype=np.uint8)
