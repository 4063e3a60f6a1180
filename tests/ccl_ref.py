"""A numpy restatement of ops/ccl.py of the reference (test-only; imports nothing from the product or the oracle).

find_components walks i = 0 .. H*W-1 in raster order; a pixel still unlabelled starts the next label and a depth-first fill from it: pop a
coordinate, label it, push its unlabelled foreground neighbours in the order up, left, right, down.  Any non-zero mask value counts as
foreground (the product's one decision beyond the reference, which takes {0, 1} only).
"""
import numpy as np

NEIGHBORS = ((-1, 0), (0, -1), (0, 1), (1, 0))


def label_image(img):
    """img [H,W] -> (labels [H,W] int32, number of components)"""
    img = np.asarray(img)
    H, W = img.shape
    todo = img != 0
    out = np.zeros((H, W), np.int32)
    label = 0
    for i in range(H * W):
        r, c = divmod(i, W)
        if not todo[r, c]:
            continue
        label += 1
        stack = [(r, c)]
        while stack:
            y, x = stack.pop()
            todo[y, x] = False
            out[y, x] = label
            for dy, dx in NEIGHBORS:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and todo[v, u]:
                    stack.append((v, u))
    return out, label


def label_components(masks):
    """masks [N,H,W] -> (labels [N,H,W] int32, counts [N] int32), image by image"""
    masks = np.asarray(masks)
    done = [label_image(m) for m in masks]
    labels = np.stack([d[0] for d in done]) if done else np.zeros(masks.shape, np.int32)
    return labels, np.array([d[1] for d in done], np.int32)
