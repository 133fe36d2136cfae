"""Pure-numpy reference of the mask post-processing (csrc/mask.hip), owned by the test suite.  No cv2, no skimage, no scipy: the
semantics are restated from the reference's source (extract_dataset.py:316-351, :394-502; inference.py:322-447), and written
STEP BY STEP as the reference writes them - three 3 x 3 iterations, never the merged radius the library runs - so that an error
in the merging shows.  test_masks_cpu.py holds this file against scipy.ndimage where scipy imports."""
import numpy as np

BG_COLOR = (127, 127, 127)


def _window(x: np.ndarray, r: int, outside: bool, combine) -> np.ndarray:
    """combine (np.logical_or / np.logical_and) of x over the (2r+1)^2 window; `outside` is the neutral value, so pixels beyond
    the image never contribute: the clipped window of cv2's default border and of skimage's closing"""
    H, W = x.shape
    pad = np.full((H + 2 * r, W + 2 * r), outside, dtype=bool)
    pad[r:r + H, r:r + W] = x
    out = np.full((H, W), outside, dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = combine(out, pad[dy:dy + H, dx:dx + W])
    return out


def dilate(x, r: int) -> np.ndarray:
    return _window(np.asarray(x).astype(bool), r, False, np.logical_or)


def erode(x, r: int) -> np.ndarray:
    return _window(np.asarray(x).astype(bool), r, True, np.logical_and)


def morph_chain(x, radii) -> np.ndarray:
    """the library's own argument, run literally: r > 0 dilates, r < 0 erodes, 0 does nothing"""
    x = np.asarray(x).astype(bool)
    for r in radii:
        if r > 0:
            x = dilate(x, r)
        elif r < 0:
            x = erode(x, -r)
    return x


def cv2_dilate(x, kernel_size: int, iterations: int) -> np.ndarray:
    """cv2.dilate(x, np.ones((k, k)), iterations=n): n passes of the k x k window"""
    x = np.asarray(x).astype(bool)
    for _ in range(iterations):
        x = dilate(x, (kernel_size - 1) // 2)
    return x


def cv2_erode(x, kernel_size: int, iterations: int) -> np.ndarray:
    x = np.asarray(x).astype(bool)
    for _ in range(iterations):
        x = erode(x, (kernel_size - 1) // 2)
    return x


def closing_square(x, k: int) -> np.ndarray:
    """skimage.morphology.closing(x, square(k))"""
    r = (k - 1) // 2
    return erode(dilate(x, r), r)


def smooth_mask(mask, kernel_size: int = 3, iterations: int = 3) -> np.ndarray:
    """extract_dataset.py:334-351, line by line"""
    closed = cv2_dilate(mask, kernel_size, iterations)
    closed = cv2_erode(closed, kernel_size, iterations)
    opened = cv2_erode(closed, kernel_size, iterations)
    return cv2_dilate(opened, kernel_size, iterations)


def label(x, connectivity: int = 8) -> np.ndarray:
    """skimage.measure.label: int32 labels 1.. numbered in raster order of each component's first pixel, 0 = background.  A plain
    host union-find over pixels."""
    x = np.asarray(x).astype(bool)
    H, W = x.shape
    parent = list(range(H * W))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    ys, xs = np.nonzero(x)
    for y, xx in zip(ys.tolist(), xs.tolist()):
        for dy, dx in back:
            yy, xn = y + dy, xx + dx
            if 0 <= yy and 0 <= xn < W and x[yy, xn]:
                a, b = find(y * W + xx), find(yy * W + xn)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.zeros((H, W), dtype=np.int32)
    names = {}
    for y, xx in zip(ys.tolist(), xs.tolist()):                 # raster order: a component is named when its first pixel is met
        root = find(y * W + xx)
        if root not in names:
            names[root] = len(names) + 1
        out[y, xx] = names[root]
    return out


def largest_component(x):
    """extract_dataset.py:437-450 -> (mask, area of the winner; 0 and an all-true mask when nothing is true)"""
    labeled = label(x)
    largest_area, largest_label = 0, 0
    areas = np.bincount(labeled.ravel())                        # region.area = the pixel count
    for lab in range(1, len(areas)):                            # regionprops: regions in label order
        area = int(areas[lab])
        if area > largest_area:
            largest_area, largest_label = area, lab
    return labeled == largest_label, largest_area


def draw_binary_mask(raw_image, binary_mask, mask_color=(0, 0, 255)) -> np.ndarray:
    """extract_dataset.py:316-331"""
    binary_mask = np.logical_not(np.asarray(binary_mask).astype(bool))
    masked = np.copy(raw_image)
    for i in range(3):
        masked[:, :, i][binary_mask] = mask_color[i]
    return masked


def create_sam_images(image, subject, body, clothes, head):
    """extract_dataset.py:394-502 after the four predictions -> (images: subject, mask, agnostic, clothes, head;
    masks: all, agnostic, clothes, head)"""
    image = np.asarray(image)[:, :, :3]
    all_masks = smooth_mask(closing_square(subject, 3))
    predicted_agnostic = smooth_mask(closing_square(body, 3))
    predicted_clothes = smooth_mask(closing_square(clothes, 3))
    predicted_head = smooth_mask(closing_square(head, 7))
    all_masks = np.logical_or(all_masks, predicted_clothes)
    all_masks = np.logical_or(all_masks, predicted_head)
    largest, _ = largest_component(all_masks)
    all_masks = smooth_mask(largest)
    unknown = np.logical_and(predicted_agnostic, predicted_clothes)
    agnostic = np.logical_and(predicted_agnostic, np.logical_not(unknown))
    clothes_mask = np.logical_and(predicted_clothes, np.logical_not(unknown))
    agnostic = np.logical_and(agnostic, all_masks)
    head_mask = np.logical_and(predicted_head, all_masks)
    clothes_mask = np.logical_and(clothes_mask, all_masks)
    images = (draw_binary_mask(image, all_masks, BG_COLOR),
              draw_binary_mask(np.zeros_like(image), agnostic, (255, 255, 255)),
              draw_binary_mask(image, agnostic, BG_COLOR),
              draw_binary_mask(image, clothes_mask, BG_COLOR),
              draw_binary_mask(image, head_mask, BG_COLOR))
    return images, (all_masks, agnostic, clothes_mask, head_mask)


def subject_image_masks(subject, body, clothes):
    """inference.py:341-420 after the three predictions -> (all, agnostic, clothes)"""
    all_masks = smooth_mask(subject)
    predicted_agnostic = smooth_mask(body)
    predicted_clothes = smooth_mask(clothes)
    all_masks = np.logical_or(all_masks, np.logical_or(predicted_agnostic, predicted_clothes))
    all_masks = smooth_mask(all_masks)
    unknown = smooth_mask(np.logical_and(predicted_agnostic, predicted_clothes))
    agnostic = np.logical_and(predicted_agnostic, np.logical_not(unknown))
    agnostic = smooth_mask(agnostic)
    return all_masks, agnostic, predicted_clothes


# ---- test inputs
def blobs(H: int, W: int, seed: int, fill: float = 0.5) -> np.ndarray:
    """a blob-like random mask: low-resolution noise enlarged by repetition, sprinkled with single-pixel noise, and with random
    first and last rows and columns (where a clipped window differs from every padded one)"""
    g = np.random.default_rng(seed)
    cell = max(1, min(H, W) // 6)
    coarse = g.random((H // cell + 1, W // cell + 1)) < fill
    x = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:H, :W].copy()
    x ^= g.random((H, W)) < 0.03
    x[0], x[-1] = g.random(W) < 0.5, g.random(W) < 0.5
    x[:, 0], x[:, -1] = g.random(H) < 0.5, g.random(H) < 0.5
    return x


def serpentine(H: int, W: int) -> np.ndarray:
    """one path, one pixel wide, over the whole image: full rows 0, 2, 4, .. joined alternately at the right and the left end"""
    x = np.zeros((H, W), dtype=bool)
    x[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        x[y, W - 1 if k % 2 == 0 else 0] = True
    return x
