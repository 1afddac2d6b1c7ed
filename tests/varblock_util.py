"""Varblock layouts that no encoder writes: the format's placement rule restated in numpy, a census of what a layout exercises in the
decoder's kernels, and the table of cases of tests/test_varblock_layouts.py (CPU) and tests/test_gpu_varblock_layouts.py (GPU).

The placement rule: the blocks of an LF group are coded as a sequence of (strategy, raw quant); each goes to the first cell, in raster
order, that no earlier block covers.  It must lie inside the frame and inside its 32x32-cell group and cover free cells only; nothing
asks for an origin that is a multiple of the block's size.  Every encoder of this project aligns its blocks, so the layouts here come
from oracle_lib.encode(varblocks=...) / (varblock_sequence=...).

A strategy's name is ROWSxCOLS in samples: DCT16X8 is one cell wide and two cells high.
"""
import numpy as np

NAMES = ["DCT8", "IDENTITY", "DCT2X2", "DCT4X4", "DCT16X16", "DCT32X32", "DCT16X8", "DCT8X16", "DCT32X8", "DCT8X32", "DCT32X16", "DCT16X32",
         "DCT4X8", "DCT8X4", "AFV0", "AFV1", "AFV2", "AFV3", "DCT64X64", "DCT64X32", "DCT32X64", "DCT128X128", "DCT128X64", "DCT64X128",
         "DCT256X256", "DCT256X128", "DCT128X256"]
S = {n: i for i, n in enumerate(NAMES)}
NUM_STRATEGIES = 27
COVERED_X = [1, 1, 1, 1, 2, 4, 1, 2, 1, 4, 2, 4, 1, 1, 1, 1, 1, 1, 8, 4, 8, 16, 8, 16, 32, 16, 32]   # width in cells
COVERED_Y = [1, 1, 1, 1, 2, 4, 2, 1, 4, 1, 4, 2, 1, 1, 1, 1, 1, 1, 8, 8, 4, 16, 16, 8, 32, 32, 16]   # height in cells
SPECIAL = (S["IDENTITY"], S["DCT2X2"], S["DCT4X4"], S["DCT4X8"], S["DCT8X4"])
MULTI_CELL = [s for s in range(NUM_STRATEGIES) if COVERED_X[s] * COVERED_Y[s] > 1]
GROUP = 32   # cells per group side
TILE = 8     # cells per side of a 64x64 reconstruction tile; the chroma-from-luma tiles are 64x64 samples too


class LayoutError(ValueError):
    """The reason is the message of the oracle's decoder for the same sequence."""


def place(sequence, w8, h8):
    """The placement rule, serially: `sequence` = [(strategy, raw_quant), ...] in coding order for a frame of one LF group.
    Returns (strategy plane with 0x80 on origins, raw quant plane), both (h8, w8), or raises LayoutError."""
    strategy = np.full((h8, w8), 0xFF, np.uint8)
    raw_quant = np.zeros((h8, w8), np.int32)
    num = 0
    for y in range(h8):
        for x in range(w8):
            if strategy[y, x] != 0xFF:
                continue
            if num >= len(sequence):
                raise LayoutError("not enough varblocks")
            s, q = sequence[num]
            if not 0 <= s < NUM_STRATEGIES:
                raise LayoutError("invalid AC strategy")
            cx, cy = COVERED_X[s], COVERED_Y[s]
            if x + cx > w8 or y + cy > h8:
                raise LayoutError("AC strategy overflows the LF group")
            if x % GROUP + cx > GROUP or y % GROUP + cy > GROUP:
                raise LayoutError("AC strategy crosses a group boundary")
            if not 1 <= q <= 256:
                raise LayoutError("quant field out of range")
            if (strategy[y:y + cy, x:x + cx] != 0xFF).any():
                raise LayoutError("overlapping varblocks")
            strategy[y:y + cy, x:x + cx] = s
            raw_quant[y:y + cy, x:x + cx] = q
            strategy[y, x] = s | 0x80
            num += 1
    if num != len(sequence):
        raise LayoutError("varblock count mismatch")
    return strategy, raw_quant


def tiling(blocks, w8, h8):
    """The strategy plane of `blocks` = [(strategy, bx, by[, raw_quant]), ...] completed with DCT8, as the oracle's writer builds it;
    ValueError when the blocks overlap, leave the frame or cross the edge of their group."""
    plane = np.full((h8, w8), 0xFF, np.uint8)
    for b in blocks:
        s, bx, by = b[:3]
        cx, cy = COVERED_X[s], COVERED_Y[s]
        if bx < 0 or by < 0 or bx + cx > w8 or by + cy > h8:
            raise ValueError("block outside the frame: %r" % (b,))
        if bx % GROUP + cx > GROUP or by % GROUP + cy > GROUP:
            raise ValueError("block crosses a group boundary: %r" % (b,))
        if (plane[by:by + cy, bx:bx + cx] != 0xFF).any():
            raise ValueError("blocks overlap: %r" % (b,))
        plane[by:by + cy, bx:bx + cx] = s
        plane[by, bx] = s | 0x80
    plane[plane == 0xFF] = S["DCT8"] | 0x80
    return plane


def coding_order(plane, raw_quant):
    """The sequence that codes a tiling: its origins in raster order (the first free cell is always the origin of the block that holds it)."""
    ys, xs = np.nonzero(plane & 0x80)
    return [(int(plane[y, x] & 0x7F), int(raw_quant[y, x])) for y, x in zip(ys, xs)]


def blocks_of(plane):
    """[(strategy, bx, by)] of a strategy plane, in raster order of origins."""
    ys, xs = np.nonzero(plane & 0x80)
    return [(int(plane[y, x] & 0x7F), int(x), int(y)) for y, x in zip(ys, xs)]


def _cell_geometry(plane):
    """Per cell: log2 of its block's width and height in cells and the cell's offset inside the block."""
    h8, w8 = plane.shape
    lcx = np.zeros((h8, w8), np.int32); lcy = np.zeros((h8, w8), np.int32)
    ix = np.zeros((h8, w8), np.int32); iy = np.zeros((h8, w8), np.int32)
    for s, bx, by in blocks_of(plane):
        cx, cy = COVERED_X[s], COVERED_Y[s]
        lcx[by:by + cy, bx:bx + cx] = cx.bit_length() - 1
        lcy[by:by + cy, bx:bx + cx] = cy.bit_length() - 1
        ix[by:by + cy, bx:bx + cx] = np.arange(cx)[None, :]
        iy[by:by + cy, bx:bx + cx] = np.arange(cy)[:, None]
    return lcx, lcy, ix, iy


def generic_tiles(plane, num_passes=1):
    """The 64x64 tiles that the tile kernel must leave to the generic kernels, as a sorted list of (tx, ty): those that hold a special
    8x8 transform, a block that does not start on a multiple of its own size, or part of a block that leaves the tile (every tile of
    a progressive frame)."""
    h8, w8 = plane.shape
    listed = set()
    for s, bx, by in blocks_of(plane):
        cx, cy = COVERED_X[s], COVERED_Y[s]
        leaves = bx // TILE != (bx + cx - 1) // TILE or by // TILE != (by + cy - 1) // TILE
        if s in SPECIAL or bx % cx or by % cy or leaves or num_passes > 1:
            for ty in range(by // TILE, (by + cy - 1) // TILE + 1):
                for tx in range(bx // TILE, (bx + cx - 1) // TILE + 1):
                    listed.add((tx, ty))
    return sorted(listed)


def gemm_tiles(plane):
    """The listed tiles that lie wholly inside one block of at least 64 points both ways: the matrix-core kernel's share."""
    out = []
    for s, bx, by in blocks_of(plane):
        cx, cy = COVERED_X[s], COVERED_Y[s]
        if cx < 8 or cy < 8:
            continue
        for ty in range(-(-by // TILE), (by + cy) // TILE):
            for tx in range(-(-bx // TILE), (bx + cx) // TILE):
                out.append((tx, ty))
    return sorted(out)


def census(plane):
    """What a decoded frame's layout exercises.  Returns a dict:
    misaligned: {strategy: subset of {"x", "y", "xy"}} over the multi-cell blocks: origin off a multiple of the width only, of the height
      only, of both;
    crosses_tile / crosses_cfl_tile: some block has cells in two 64x64 tiles / in two chroma-from-luma tiles (the same grid: both are
      64x64 samples); touches_partial_tile: a multi-cell block has cells in a tile that the frame's right or bottom edge cuts;
    pairs_v: {(log2 length left, log2 length right)} over the 2x2-cell sub-blocks at even cell coordinates: the vertical transform
      lengths (8 << log2 of the height in cells) of the sub-block's upper two cells, the inputs of the tile kernel's vertical pass;
    pairs_h: {(top, bottom)}: the horizontal lengths of its left two cells.  Lengths above 64 are left out (log2 3..6 remain)."""
    h8, w8 = plane.shape
    lcx, lcy, _, _ = _cell_geometry(plane)
    out = dict(misaligned={}, crosses_tile=False, crosses_cfl_tile=False, touches_partial_tile=False, pairs_v=set(), pairs_h=set())
    for s, bx, by in blocks_of(plane):
        cx, cy = COVERED_X[s], COVERED_Y[s]
        if cx * cy == 1:
            continue
        mx, my = bx % cx != 0, by % cy != 0
        if mx or my:
            out["misaligned"].setdefault(s, set()).add("xy" if mx and my else ("x" if mx else "y"))
        if bx // TILE != (bx + cx - 1) // TILE or by // TILE != (by + cy - 1) // TILE:
            out["crosses_tile"] = out["crosses_cfl_tile"] = True
        if (w8 % TILE and (bx + cx - 1) // TILE == w8 // TILE) or (h8 % TILE and (by + cy - 1) // TILE == h8 // TILE):
            out["touches_partial_tile"] = True
    for y in range(0, h8 - 1, 2):
        for x in range(0, w8 - 1, 2):
            if lcy[y, x] <= 3 and lcy[y, x + 1] <= 3:
                out["pairs_v"].add((3 + int(lcy[y, x]), 3 + int(lcy[y, x + 1])))
            if lcx[y, x] <= 3 and lcx[y + 1, x] <= 3:
                out["pairs_h"].add((3 + int(lcx[y, x]), 3 + int(lcx[y + 1, x])))
    return out


def free_runs(sequence, w8, h8):
    """Per row, the runs (first cell, length) of cells that are free when the placement reaches the row: what the row-parallel placement
    kernel sees in its coverage words."""
    plane, _ = place(sequence, w8, h8)
    iy = _cell_geometry(plane)[3]
    rows = []
    for y in range(h8):
        free = iy[y] == 0   # covered from above: the cells of blocks that started in an earlier row
        runs, x = [], 0
        while x < w8:
            if free[x]:
                x0 = x
                while x < w8 and free[x]:
                    x += 1
                runs.append((x0, x - x0))
            else:
                x += 1
        rows.append(runs)
    return rows


def allowed_classes(s):
    """The misalignment classes the group rule leaves a strategy: a side of one cell is always aligned, a side of 32 cells cannot move."""
    cx, cy = COVERED_X[s], COVERED_Y[s]
    mx, my = 1 < cx < GROUP, 1 < cy < GROUP
    return {c for c, ok in (("x", mx), ("y", my), ("xy", mx and my)) if ok}


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, name, w, h, blocks):
        self.name, self.w, self.h = name, w, h
        self.w8, self.h8 = (w + 7) // 8, (h + 7) // 8
        self.blocks = [tuple(b) if len(b) == 4 else tuple(b) + (12 + (5 * i) % 9,) for i, b in enumerate(blocks)]   # raw quants that differ
        self.plane = tiling(self.blocks, self.w8, self.h8)

    def __repr__(self):
        return self.name


def _first_fit(plane, s, cls):
    """The first origin in raster order where strategy `s` is free, legal and misaligned as `cls` says ("", "x", "y", "xy")."""
    h8, w8 = plane.shape
    cx, cy = COVERED_X[s], COVERED_Y[s]
    for y in range(h8 - cy + 1):
        for x in range(w8 - cx + 1):
            if (x % cx != 0) != ("x" in cls) or (y % cy != 0) != ("y" in cls):
                continue
            if x % GROUP + cx > GROUP or y % GROUP + cy > GROUP:
                continue
            if (plane[y:y + cy, x:x + cx] == 0xFF).all():
                return x, y
    raise ValueError("no room for %s %r" % (NAMES[s], cls))


def _small_shifts():
    """Every multi-cell strategy of at most 64 points misaligned in x only, in y only and in both (as far as it has the side for it),
    packed first-fit into 272x272, the cells left over cycling through DCT8 and the five special 8x8 transforms."""
    w8 = h8 = 34
    plane = np.full((h8, w8), 0xFF, np.uint8)
    blocks = []

    def put(s, x, y):
        plane[y:y + COVERED_Y[s], x:x + COVERED_X[s]] = s
        blocks.append((s, x, y))
    put(S["DCT16X16"], 7, 7)      # touches four tiles
    put(S["DCT32X8"], 20, 6)      # one cell wide, rows 6..9: crosses one tile edge
    put(S["DCT8X32"], 14, 0)      # cells 14..17 of row 0: crosses one tile edge
    small = [s for s in MULTI_CELL if COVERED_X[s] <= 8 and COVERED_Y[s] <= 8]
    for s in sorted(small, key=lambda s: -COVERED_X[s] * COVERED_Y[s]):
        for cls in ("x", "y", "xy"):
            if cls in allowed_classes(s):
                put(s, *_first_fit(plane, s, cls))
    cycle = [S["DCT8"], S["IDENTITY"], S["DCT2X2"], S["DCT4X4"], S["DCT4X8"], S["DCT8X4"], S["DCT8"]]
    for y in range(h8):
        for x in range(w8):
            if plane[y, x] == 0xFF:
                put(cycle[(x + 2 * y) % 7], x, y)
    return Case("small-shifts", 272, 272, blocks)


def _split_rows():
    """Blocks of heights 1, 2 and 4 cells side by side, each row filled left to right with the next strategy of a cycle that fits: the
    rows below a first row are cut into many runs of free cells by what hangs from above, and the next blocks fill the gaps."""
    w8, h8 = 34, 12
    plane = np.full((h8, w8), 0xFF, np.uint8)
    cycle = [S["DCT32X8"], S["DCT8X16"], S["DCT16X8"], S["DCT8"], S["DCT16X16"], S["DCT16X32"], S["DCT8"], S["DCT32X16"], S["DCT8X32"],
             S["DCT16X8"], S["DCT32X32"], S["DCT8"]]
    blocks, k = [], 0
    for y in range(h8):
        for x in range(w8):
            if plane[y, x] != 0xFF:
                continue
            for t in range(len(cycle)):
                s = cycle[(k + t) % len(cycle)]
                cx, cy = COVERED_X[s], COVERED_Y[s]
                if x + cx <= w8 and y + cy <= h8 and x % GROUP + cx <= GROUP and (plane[y:y + cy, x:x + cx] == 0xFF).all():
                    break
            k += t + 1
            plane[y:y + cy, x:x + cx] = s
            blocks.append((s, x, y))
    return Case("split-rows", 272, 96, blocks)


def _aligned_pairs():
    """Aligned blocks only.  The vertical pass of the tile kernel compares the two upper cells of a 16x16 sub-block: two neighbours of
    different heights are both one cell wide there, since a wider aligned block holds both cells.  One-cell-wide strategies are 8, 16 and
    32 samples high, so an aligned layout can show the nine pairs of those lengths and (64, 64); (64, other) needs a block 64 high and
    one cell wide, which the format does not have.  The horizontal pass likewise."""
    blocks = []
    col = {3: S["DCT8"], 4: S["DCT16X8"], 5: S["DCT32X8"]}
    row = {3: S["DCT8"], 4: S["DCT8X16"], 5: S["DCT8X32"]}
    k = 0
    for a in (3, 4, 5):
        for b in (3, 4, 5):
            blocks += [(col[a], 2 * k, 0), (col[b], 2 * k + 1, 0)]
            blocks += [(row[a], 4 * (k % 5), 4 + 2 * (k // 5)), (row[b], 4 * (k % 5), 5 + 2 * (k // 5))]
            k += 1
    blocks += [(S["DCT64X64"], 0, 8), (S["DCT32X32"], 8, 8), (S["DCT64X32"], 12, 8), (S["DCT32X64"], 8, 16), (S["DCT16X16"], 8, 12)]
    return Case("aligned-pairs", 160, 160, blocks)


ALIGNED_PAIRS = {(a, b) for a in (3, 4, 5) for b in (3, 4, 5)} | {(6, 6)}


def _odd_pairs():
    """The length pairs an aligned layout cannot show, (64, other) and (other, 64), from blocks 64 long whose edge falls inside a 16x16
    sub-block.  Such tiles go to the generic kernels; the case completes the census of 16 + 16 pairs over the table."""
    blocks = []
    col = {3: S["DCT8"], 4: S["DCT16X8"], 5: S["DCT32X8"]}
    row = {3: S["DCT8"], 4: S["DCT8X16"], 5: S["DCT8X32"]}
    for k, a in enumerate((3, 4, 5)):
        blocks += [(col[a], 6 * k, 0), (S["DCT64X32"], 6 * k + 1, 0), (col[a], 6 * k + 5, 0)]
        blocks += [(row[a], 0, 8 + 6 * k), (S["DCT32X64"], 0, 9 + 6 * k), (row[a], 0, 13 + 6 * k)]
    return Case("odd-pairs", 144, 208, blocks)


def _one_shift(s, cls):
    """One block of strategy `s` misaligned as `cls`, in the smallest frame that holds it with a cell to spare."""
    cx, cy = COVERED_X[s], COVERED_Y[s]
    bx, by = (3 if "x" in cls else 0), (3 if "y" in cls else 0)
    return Case("shift-%s-%s" % (NAMES[s], cls), 8 * (bx + cx + 1), 8 * (by + cy + 1), [(s, bx, by)])


def _cases():
    c = [
        # the block's last cell alone in tile (1, 1): GemmTile's case
        Case("tile-corner-64", 72, 72, [(S["DCT64X64"], 1, 1)]),
        Case("odd-64s", 136, 200, [(S["DCT64X64"], 1, 1), (S["DCT64X32"], 9, 3), (S["DCT32X64"], 3, 13), (S["DCT64X32"], 13, 11),
                                   (S["DCT32X64"], 1, 19), (S["IDENTITY"], 0, 0), (S["DCT4X8"], 16, 24)]),
        # tile (1, 1) wholly inside (matrix cores), tile (2, 2) holds one cell of it (must not)
        Case("big-128", 272, 272, [(S["DCT128X128"], 1, 1)]),
        # misaligned in their short direction only
        Case("long-short", 264, 208, [(S["DCT128X64"], 3, 0), (S["DCT64X128"], 16, 17)]),
        # the 16-cell side at offset 3; the 32-cell side cannot move: (x % 32) + 32 <= 32
        Case("tall-256", 160, 264, [(S["DCT256X128"], 3, 0)]),
        Case("wide-256", 264, 160, [(S["DCT128X256"], 0, 3)]),
        _small_shifts(), _split_rows(), _aligned_pairs(), _odd_pairs(),
        # shifted blocks that stay inside their tile, with DCT8 around them: only the misalignment itself lists tiles (0, 0), (1, 0) and
        # (0, 1); tile (1, 1) is aligned and stays with the tile kernel
        Case("tile-interior", 128, 128, [(S["DCT16X16"], 1, 1), (S["DCT16X8"], 4, 1), (S["DCT8X16"], 5, 4),
                                        (S["DCT32X32"], 9, 1), (S["DCT32X16"], 13, 3),
                                        (S["DCT16X32"], 1, 9), (S["DCT32X8"], 6, 9), (S["DCT8X32"], 1, 12),
                                        (S["DCT16X16"], 8, 8), (S["DCT16X16"], 10, 10), (S["DCT32X32"], 12, 12)]),
    ]
    for s in MULTI_CELL:
        if COVERED_X[s] >= 8 or COVERED_Y[s] >= 8:     # the strategies too large for small-shifts
            have = set()
            for k in c:
                have |= census(k.plane)["misaligned"].get(s, set())
            c += [_one_shift(s, cls) for cls in ("x", "y", "xy") if cls in allowed_classes(s) - have]
    return c


# Writer soundness (tests/test_varblock_layouts.py::test_writer_soundness): mean absolute error of the oracle's decode against the source
# picture smooth(w, h), distance 1.0, as a ratio to the same picture written with DCT8 only - over the whole picture, and over the
# samples of each named multi-cell block (the DCT8 error of a block floored at 0.25 grey levels).  A block whose coefficients went to
# the wrong place costs an error of the order of the picture's contrast, tens of grey levels against a coding error below one: a ratio
# above 10 for that block.  Measured on the CPU, whole picture / worst block:
#   tile-corner-64 0.87 / 0.83   odd-64s 0.93 / 1.00      big-128 0.96 / 0.82      long-short 0.95 / 0.84   tall-256 0.88 / 0.84
#   wide-256 0.86 / 0.82         small-shifts 1.14 / 1.34 split-rows 0.90 / 1.34   aligned-pairs 0.90 / 1.35  odd-pairs 0.94 / 1.14
#   tile-interior 0.97 / 1.07
#   shift-DCT128X128-x 0.90 / 0.87, -y 0.87 / 0.81   shift-DCT128X64-y 0.85 / 0.78, -xy 0.90 / 0.81   shift-DCT64X128-x 0.89 / 0.85, -xy 0.91 / 0.84
# Large transforms code this content a little better than DCT8; the named blocks' raw quants (12..20 against the writer's 16..24) and
# the special 8x8 transforms of small-shifts cost a little.  The bounds leave room for that and none for a misplaced block.
MAX_ERROR_RATIO = 1.5
MAX_BLOCK_ERROR_RATIO = 2.0
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _seq(plane, q=16):
    return [(s, q) for s, _, _ in blocks_of(plane)]


def _invalid():
    """(name, w, h, sequence, the oracle decoder's reason).  Each sequence is valid up to one block."""
    D, out = S["DCT8"], []
    # a tall block from row 0; the wide block at the start of row 1 needs cells 0..3, and cell 2 is the tall block's.  The rest is what a
    # decoder that did not notice would go on to accept: three more blocks in row 1, eight in row 2.
    out.append(("overlap", 64, 24, [(D, 16), (D, 16), (S["DCT16X8"], 16)] + [(D, 16)] * 5 + [(S["DCT8X32"], 16)] + [(D, 16)] * 11, "overlapping varblocks"))
    out.append(("group-edge-x", 272, 16, [(D, 16)] * 31 + [(S["DCT8X16"], 16)] + [(D, 16)] * 35, "AC strategy crosses a group boundary"))
    out.append(("group-edge-y", 16, 272, [(D, 16)] * 62 + [(S["DCT16X8"], 16)] + [(D, 16)] * 4, "AC strategy crosses a group boundary"))
    out.append(("right-edge", 24, 16, [(D, 16), (D, 16), (S["DCT8X16"], 16), (D, 16), (D, 16)], "AC strategy overflows the LF group"))
    out.append(("bottom-edge", 16, 24, [(D, 16)] * 4 + [(S["DCT16X8"], 16), (D, 16)], "AC strategy overflows the LF group"))
    valid = _seq(tiling([(S["DCT16X16"], 1, 0), (S["DCT8X16"], 1, 2)], 4, 3))
    out.append(("count-short", 32, 24, valid[:-1], "not enough varblocks"))     # the frame's last cell stays free
    out.append(("count-long", 32, 24, valid + [(D, 16)], "varblock count mismatch"))
    out.append(("strategy-27", 32, 24, valid[:3] + [(27, 16)] + valid[4:], "invalid AC strategy"))
    return out


INVALID = _invalid()


def smooth(w, h, nch=4):
    """A smooth picture with contrast (a few slow sinusoids per channel, opaque alpha): large transforms code it well, and a
    coefficient in the wrong place shows."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 4), np.uint8)
    for c, (fx, fy, ph) in enumerate(((0.021, 0.013, 0.3), (0.011, 0.027, 1.1), (0.017, 0.019, 2.3))):
        v = 128 + 70 * np.sin(fx * x + ph) * np.cos(fy * y - ph) + 40 * np.sin(0.031 * (x + y) + c)
        img[..., c] = np.clip(np.rint(v), 0, 255)
    img[..., 3] = 255
    return np.ascontiguousarray(img[..., :nch])
