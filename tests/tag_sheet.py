"""Tag sheets: a white gray image with upright tags on a regular grid, for frames with hundreds of detections.

A tag is `family.grid(id)` with `cell` pixels per cell; tags are `gap` pixels apart and from the image's edge.  The CPU
oracle finds exactly the tags placed (checked in tests/test_dedup_ref.py for the sheets the GPU tests use), at decimate 1
with 4-pixel cells and at decimate 2 with 6-pixel cells."""
import numpy as np


def capacity(family, width, height, cell, gap):
    pitch = family.total_width * cell + gap
    return ((width - gap) // pitch) * ((height - gap) // pitch)


def tag_sheet(family, width, height, cell, gap, n=None, ids=lambda k: k % 512):
    """(height, width) uint8 with the first n grid positions (default: all) holding tags ids(0), ids(1), ..., row by row"""
    side = family.total_width * cell
    pitch = side + gap
    cols = (width - gap) // pitch
    total = capacity(family, width, height, cell, gap)
    n = total if n is None else n
    assert 0 <= n <= total, (n, total)
    img = np.full((height, width), 255, dtype=np.uint8)
    ones = np.ones((cell, cell), dtype=np.uint8)
    for k in range(n):
        y, x = gap + (k // cols) * pitch, gap + (k % cols) * pitch
        img[y:y + side, x:x + side] = np.kron(family.grid(ids(k)), ones) * 255
    return img
