"""A synthetic Vimeo-90K septuplet tree and a stub enhancer for the tests of the video-enhancement loop
(networks/septuplet_io.py): tests/test_septuplet_host.py on the CPU, tests/test_gpu_stack.py with the pixel work on the
device.  The stub is arithmetic that numpy repeats bit for bit (single float32 operations in one order, constants that are
numbers of float32), so the expected bytes are computed here without the loop's own padding, cropping or rounding."""
import os

import numpy as np
import torch

# (sequence/clip, h, w): two small clips, and one whose sides are multiples of 128 already (the 32 + 32 branch)
CLIPS = (("00001/0001", 24, 40), ("00001/0002", 24, 40), ("00002/0001", 128, 128))


def write_tree(root, write_png, seed=5):
    """<root>/input/<clip>/im1..7.png (a noisy septuplet) and <root>/target/<clip>/im4.png; -> {clip: (frames, target)}"""
    rng = np.random.default_rng(seed)
    made = {}
    for clip, h, w in CLIPS:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 150 * np.sin(xx / (5.0 + c) + k) * np.cos(yy / (7.0 - c)) for c, k in ((0, 0.3), (1, 1.1), (2, 2.0))], 2)
        target = np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
        frames = [np.clip(np.roll(base, k - 3, axis=1) + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8) for k in range(7)]
        for d, names, imgs in (("input", ["im%d.png" % (k + 1) for k in range(7)], frames), ("target", ["im4.png"], [target])):
            os.makedirs(os.path.join(root, d, clip), exist_ok=True)
            for name, img in zip(names, imgs):
                write_png(os.path.join(root, d, clip, name), img)
        made[clip] = (frames, target)
    return made


def _ramp(h, w):
    return ((np.arange(w)[None, :] + 2 * np.arange(h)[:, None]) % 16).astype(np.float32) / np.float32(64)


class StubEnhancer(torch.nn.Module):
    """seven [1, 3, H, W] frames -> 1.25 * (x3 / 2 + x2 / 4 + x4 / 4) - 1 / 8 + a ramp over the PADDED grid (so a wrong crop
    shows); leaves [0, 1] on both sides (so the clip shows); records the shapes it was called with"""

    def __init__(self):
        super().__init__()
        self.shapes = []

    def forward(self, xs, y=None):
        assert len(xs) == 7 and all(x.shape == xs[0].shape and x.dtype == torch.float32 for x in xs)
        self.shapes.append(tuple(xs[0].shape))
        h, w = xs[0].shape[2:]
        ramp = torch.from_numpy(_ramp(h, w)).to(xs[0].device)
        return (xs[3] * 0.5 + xs[2] * 0.25 + xs[4] * 0.25) * 1.25 - 0.125 + ramp


def pad_rule(n):
    """demo_Vimeo_VE.py:115-131, restated: (before, after) of one side"""
    if n % 128 == 0:
        return 32, 32
    total = (n // 128 + 1) * 128 - n
    return total // 2, total - total // 2


def expected_centre(frames):
    """what the loop must write for these seven uint8 [h, w, 3] frames under StubEnhancer"""
    h, w, _c = frames[0].shape
    (top, bottom), (left, right) = pad_rule(h), pad_rule(w)
    f32 = np.float32
    x2, x3, x4 = (np.pad(np.transpose(frames[k], (2, 0, 1)).astype(f32) / f32(255), ((0, 0), (top, bottom), (left, right)),
                         mode="edge") for k in (2, 3, 4))
    y = (x3 * f32(0.5) + x2 * f32(0.25) + x4 * f32(0.25)) * f32(1.25) - f32(0.125) + _ramp(h + top + bottom, w + left + right)
    y = y[:, top:top + h, left:left + w]
    return np.ascontiguousarray(np.transpose(np.round(f32(255) * np.clip(y, f32(0), f32(1))), (1, 2, 0)).astype(np.uint8))


def padded_shape(h, w):
    return (1, 3, h + sum(pad_rule(h)), w + sum(pad_rule(w)))
