"""Writing recorded frames to disk without a video codec: an animated GIF through PIL when it is importable, the raw
(T, H, W, 4) uint8 array as .npy otherwise."""
import os

import numpy as np


def save_frames(frames, path, fps=50.0):
    """Write `frames` (a list or array of (H, W, 4) or (H, W, 3) uint8) as `path` (.gif).  Returns the path
    written: `path`, or the same name with .npy when PIL is missing."""
    arr = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]), dtype=np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        out = os.path.splitext(path)[0] + ".npy"
        np.save(out, arr)
        return out
    imgs = [Image.fromarray(f[..., :3]) for f in arr]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
    return path
