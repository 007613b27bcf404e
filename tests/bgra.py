"""BGRA keyframes with a hostile alpha plane -- test code only.

The tracker hands the fusion side 8UC4 frames and the maps drop the alpha byte in the warp's gather.  A gather that
slips by a byte, or a tap that reads the alpha byte where it wants a colour, shows only if the alpha differs from the colours around it:
with_alpha() picks every pixel's alpha at least ALPHA_GAP away from each of the pixel's three colour values, whatever the frame holds
("const" and "white" included), and padded() / padded_device() lay such a frame out with rows that are no multiple of 4 bytes apart."""
import numpy as np

ALPHA_CANDIDATES = (255, 0, 128, 64)
ALPHA_GAP = 32              # the candidates are at least 64 apart, so one colour value blocks at most one of them: of four, one remains
PAD_BYTE = 0xA5
PADS = (6, 90)              # bytes between rows; with 6, rows start at 2 mod 4: no row but the first is 4-byte aligned


def with_alpha(bgr, k):
    """H x W x 4 uint8: bgr and an alpha plane that takes, per pixel, the first of ALPHA_CANDIDATES at least ALPHA_GAP away from each
    of the pixel's three colour values.  The candidate order is rotated by k, so that consecutive keyframes do not share a plane, and
    by x + y as well: on a frame of one colour the plane would otherwise be one value too, and a gather that slips onto it would see
    another constant frame -- the same (zero) Laplacian on every level but the top one."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    n = len(ALPHA_CANDIDATES)
    y, x = np.mgrid[0:bgr.shape[0], 0:bgr.shape[1]]
    first = (x + y + k) % n
    v = np.arange(256)
    blocks = sum(((np.abs(v - a) < ALPHA_GAP) << r) for r, a in enumerate(ALPHA_CANDIDATES)).astype(np.uint8)   # per colour value: the candidates it blocks
    blocked = blocks[bgr[:, :, 0]] | blocks[bgr[:, :, 1]] | blocks[bgr[:, :, 2]]
    pick = np.zeros((1 << n, n), np.uint8)                  # (set of blocked candidates, first candidate of the order) -> alpha
    for b in range((1 << n) - 1):
        for f in range(n):
            pick[b, f] = next(ALPHA_CANDIDATES[(f + i) % n] for i in range(n) if not (b >> ((f + i) % n)) & 1)
    assert blocked.max() < (1 << n) - 1                     # one always remains
    alpha = pick[blocked, first]
    return np.dstack([bgr, alpha])


def apart(bgra):
    """the smallest |alpha - colour| of a BGRA frame"""
    c = bgra.astype(np.int16)
    return int(np.abs(c[:, :, :3] - c[:, :, 3:]).min())


def padded(bgra, pad_bytes):
    """A view with strides (cols * 4 + pad_bytes, 4, 1) over a wider byte buffer whose padding bytes are PAD_BYTE (rows * step
    bytes: the view's first pixel is its first byte)"""
    rows, cols, cn = bgra.shape
    assert cn == 4 and bgra.dtype == np.uint8
    step = cols * 4 + pad_bytes
    buf = np.full(rows * step, PAD_BYTE, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, shape=(rows, cols, 4), strides=(step, 4, 1))
    view[:] = bgra
    return view


def frame_bytes(view):
    """the caller's bytes from the view's first pixel to its last, padding between the rows included: what the map keeps of a frame"""
    rows, cols, cn = view.shape
    n = (rows - 1) * view.strides[0] + cols * cn
    return np.lib.stride_tricks.as_strided(view, shape=(n,), strides=(1,))


def padded_device(bgra, pad_bytes):
    """(uint8 device tensor of rows * step bytes in the layout of padded(), step): for feed_device(t.data_ptr(), ..., step=step, channels=4)"""
    import torch
    view = padded(bgra, pad_bytes)
    rows, step = view.shape[0], view.strides[0]
    host = np.lib.stride_tricks.as_strided(view, shape=(rows * step,), strides=(1,))
    return torch.from_numpy(np.array(host)).cuda(), step
