"""What the page-stage GPU tests (tests/test_<stage>_gpu.py) share: a page placed inside a larger buffer, the poisoned output buffer and the host
buffer it must equal, garbage scratch, word outputs followed by sentinels, the tile sizes of a .hip file.  The fill, the poison, the tail, the scratch floor, the guard
count and the sentinel decide what an out-of-bounds read or write would hit, so every file passes its own: place keeps only the defaults
that the files' own helpers shared (fill 0, a 16-byte tail), and expect_placed has none.  The numpy half (placed_bytes, expect_placed,
csrc_constants) needs no device; tests/test_page_harness_cpu.py checks it."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torch-attention-ocr_amd", "csrc")


def placed_bytes(page, pitch=None, offset=0, fill=0, tail=16, elem=1):
    """the page inside a larger host buffer: rows `pitch` bytes apart, starting `offset` bytes in, `tail` bytes behind the last row's pitch;
    every other byte is `fill`.  `page` is (H, W) bytes, or (H, W, elem) for pixels of `elem` bytes."""
    H, row = page.shape[0], page.shape[1] * elem
    pitch = pitch or row
    buf = np.full(offset + H * pitch + tail, fill, np.uint8)
    np.lib.stride_tricks.as_strided(buf[offset:], (H, row), (pitch, 1))[:] = page.reshape(H, row)
    return buf


def place(cuda, page, pitch=None, offset=0, fill=0, tail=16, elem=1):
    """placed_bytes on the device: (the buffer, which the caller keeps alive, the page's address, its pitch)."""
    import torch
    dev = torch.from_numpy(placed_bytes(page, pitch, offset, fill, tail, elem)).to(cuda)
    return dev, dev.data_ptr() + offset, pitch or page.shape[1] * elem


def poisoned(cuda, n_bytes, poison):
    """a device output buffer of n_bytes, every byte `poison`."""
    import torch
    return torch.full((n_bytes,), poison, dtype=torch.uint8, device=cuda)


def expect_placed(want, out_pitch=None, out_offset=0, *, poison, tail):
    """the host buffer a whole poisoned output buffer must equal: `want` strided in, every byte around it still `poison`."""
    return placed_bytes(want, out_pitch, out_offset, fill=poison, tail=tail)


def garbage_scratch(cuda, need_bytes, floor_bytes=0):
    """int64 scratch of at least need_bytes and at least floor_bytes, every word -1."""
    import torch
    return torch.full(((max(need_bytes, floor_bytes) + 7) // 8,), -1, dtype=torch.int64, device=cuda)


def guarded_words(cuda, n, guard, sentinel, dtype, width=None):
    """a word output of n entries (rows of `width` words, if given) and `guard` more behind them, all `sentinel`: the guard entries must
    keep it, so that a write past the end lands in words the caller checks, not in the allocator's slack."""
    import torch
    return torch.full((n + guard,) if width is None else (n + guard, width), sentinel, dtype=dtype, device=cuda)


def csrc_constants(file_name, names):
    """{name: int} from the `constexpr int NAME = N;` lines of a file under csrc/; a name the file does not define is an error."""
    src = open(os.path.join(CSRC, file_name)).read()
    found = {n: int(v) for n, v in re.findall(r"constexpr int (\w+) = (\d+);", src) if n in names}
    missing = [n for n in names if n not in found]
    if missing:
        raise KeyError(f"{file_name} defines no constexpr int {', '.join(missing)}")
    return found


def same_reading(a, b):
    np.testing.assert_array_equal(a.boxes, b.boxes)
    np.testing.assert_array_equal(a.line, b.line)
    np.testing.assert_array_equal(a.labels, b.labels)
    assert a.text == b.text and a.n_lines == b.n_lines


def corner_pixels(boxes):
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    return (np.stack([b[:, 0], b[:, 2] - 1, b[:, 2] - 1, b[:, 0]], 1).astype(np.float64),
            np.stack([b[:, 1], b[:, 1], b[:, 3] - 1, b[:, 3] - 1], 1).astype(np.float64))
