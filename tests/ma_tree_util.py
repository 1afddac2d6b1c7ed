"""Explicit MA trees for the Modular decode paths: a seeded generator of named tree families (oracle_lib.encode(tree=...)), the
geometry of a lossless frame's Modular streams, and a restatement of the rules by which the decoder picks a path for a channel.

The decoder's choice cannot be observed from outside; classify() says which path a case is BUILT to reach, by the rules of
csrc/entropy_kernels.hip (ClassifyChannel, RowNode, SkewPred, kCarryInts, DecodeChannelLane) and csrc/modular_uniform.h
(ModularChannelUniform: kUniMaxProps, the 32 / 16 threshold lanes of a slot, kUniGridCells in csrc/dev_types.h), written out here on
their own.  The labels hold for the launch shape with one section per wavefront; the per-lane walk (ModularChannel) has no grid, there
every channel that is not constant or row-static is walked."""
import numpy as np

# ---------------------------------------------------------------- the decoder's constants, by their names in the headers
K_UNI_MAX_PROPS = 4        # modular_uniform.h: kUniMaxProps
K_UNI_GRID_CELLS = 2048    # dev_types.h: kUniGridCells
K_SLOT_LANES_32 = 32       # modular_uniform.h: layout32, two slots of 32 lanes (at most 2 properties)
K_SLOT_LANES_16 = 16       # ... four slots of 16 lanes
K_LEAF_LANES = 64          # modular_uniform.h: leaf_in_lanes, cells <= 64
K_MAX_COLLECTED = 63       # modular_uniform.h: nthr[k] >= 63 gives up while collecting
K_CARRY_INTS = 1024        # entropy_kernels.hip: kCarryInts
K_NUM_QUANT_TABLES = 17    # dev_types.h: kNumQuantTables (stream ids of the pass groups start after them)
GROUP_DIM = 256            # the oracle writes lossless frames with group_size_shift 1
LF_GROUP_DIM = 8 * GROUP_DIM
SKEW_PREDS = (0, 1, 2, 5)  # entropy_kernels.hip: SkewPred

LABELS = ("const", "row-static", "grid-lanes", "grid-lds", "walk")
SIZES = [(1, 1), (2, 3), (63, 5), (65, 66), (130, 67), (257, 70), (70, 257)]


# ---------------------------------------------------------------- trees
def L(pred, off=0, mul=1):
    return ("L", pred, off, mul)


def S(prop, val, gt, le):
    return ("S", prop, val, gt, le)


def flatten(t):
    """Nested tuples -> the node list encode() takes (parents before children)."""
    nodes = []

    def put(n):
        i = len(nodes)
        nodes.append(None)
        if n[0] == "L":
            nodes[i] = [-1, 0, 0, 0, n[1], n[2], n[3]]
        else:
            a = put(n[3])
            b = put(n[4])
            nodes[i] = [n[1], n[2], a, b, 0, 0, 1]
        return i
    put(t)
    return nodes


def buckets(prop, thrs, subs):
    """A balanced tree over the sorted thresholds: subs[k] is reached by values > thrs[k - 1] and <= thrs[k]."""
    assert len(subs) == len(thrs) + 1 and list(thrs) == sorted(thrs)

    def build(lo, hi):
        if lo == hi:
            return subs[lo]
        mid = (lo + hi) // 2
        return S(prop, thrs[mid], build(mid + 1, hi), build(lo, mid))
    return build(0, len(thrs))


class Leaves:
    """Hands out leaves that cycle through a list of (predictor, offset, multiplier)."""

    def __init__(self, forms, start=0):
        self.forms = [f if isinstance(f, tuple) else (f, 0, 1) for f in forms]
        self.k = start

    def __call__(self):
        f = self.forms[self.k % len(self.forms)]
        self.k += 1
        return L(*f)


def nest(levels, leaf):
    """levels: [(property, thresholds), ...].  The first property's buckets end in leaves, except the one around zero (the bucket
    of the first threshold >= 0), which goes on with the next property: few nodes, but the grid of the whole tree is the full product."""
    prop, thrs = levels[0]
    mid = next((k for k, t in enumerate(thrs) if t >= 0), len(thrs))
    subs = [leaf() for _ in range(len(thrs) + 1)]
    if len(levels) > 1:
        subs[mid] = nest(levels[1:], leaf)
    return buckets(prop, thrs, subs)


def uses_wp(nodes):
    return any(n[0] == 15 or (n[0] < 0 and n[4] == 6) for n in nodes)


# ---------------------------------------------------------------- which path a channel is built to reach
def _row_leaf(nodes, chan, sid, y):
    """RowNode: follows properties 0, 1, 2; returns (node index, whether property 2 was looked at)."""
    i, used_y = 0, False
    while 0 <= nodes[i][0] <= 2:
        p, v = nodes[i][0], nodes[i][1]
        used_y |= p == 2
        i = nodes[i][2] if (chan, sid, y)[p] > v else nodes[i][3]
    return i, used_y


def classify(nodes, chan, sid, w, h, one_symbol=()):
    """one_symbol: indices of the leaves whose context the case is built to fill with a single residual."""
    if not uses_wp(nodes):   # DecodeChannelLane: a tree that uses the weighted predictor anywhere keeps every channel per-sample
        static, const, needs_n = True, True, False
        for y in range(h):
            i, used_y = _row_leaf(nodes, chan, sid, y)
            if nodes[i][0] >= 0 or nodes[i][4] not in SKEW_PREDS:
                static = False
                break
            needs_n |= nodes[i][4] in (2, 5)
            const &= nodes[i][4] == 0 and i in one_symbol
            if not used_y:
                break
        if static and not (needs_n and h > 64 and w > K_CARRY_INTS):
            return "const" if const else "row-static"
    # ModularChannelUniform: the static nodes on top, then a walk of the subtree that follows the live child of a static node
    props, stack = {}, [0]
    while stack:
        i = stack.pop()
        p, v = nodes[i][0], nodes[i][1]
        if p < 0:
            continue
        if p in (0, 1):
            stack.append(nodes[i][2] if (chan, sid)[p] > v else nodes[i][3])
            continue
        if p > 15:
            return "walk"
        if p not in props:
            if len(props) == K_UNI_MAX_PROPS:
                return "walk"
            props[p] = set()
        if v not in props[p]:
            if len(props[p]) >= K_MAX_COLLECTED:
                return "walk"
            props[p].add(v)
        stack += [nodes[i][3], nodes[i][2]]
    most = max([len(t) for t in props.values()] + [0])
    if most > (K_SLOT_LANES_32 if len(props) <= 2 else K_SLOT_LANES_16):
        return "walk"
    cells = 1
    for t in props.values():
        cells *= len(t) + 1
    if cells > K_UNI_GRID_CELLS:
        return "walk"
    return "grid-lanes" if cells <= K_LEAF_LANES else "grid-lds"


# ---------------------------------------------------------------- geometry of a lossless frame's streams
def _default_squeeze(chans):
    """DefaultSqueezeParams + MetaSqueeze on a list of [w, h, hshift, vshift]."""
    w, h = chans[0][0], chans[0][1]
    steps = []
    if len(chans) > 2 and chans[1][:2] == [w, h]:
        steps += [(True, False, 1, 2), (False, False, 1, 2)]
    n = len(chans)
    if h > w and h > 8:
        steps.append((False, True, 0, n))
        h = (h + 1) // 2
    while w > 8 or h > 8:
        if w > 8:
            steps.append((True, True, 0, n))
            w = (w + 1) // 2
        if h > 8:
            steps.append((False, True, 0, n))
            h = (h + 1) // 2
    for horizontal, in_place, begin, num in steps:
        end = begin + num - 1
        offset = end + 1 if in_place else len(chans)
        for c in range(begin, end + 1):
            cw, ch, hs, vs = chans[c]
            if horizontal:
                chans[c] = [(cw + 1) // 2, ch, hs + 1, vs]
                res = [cw - (cw + 1) // 2, ch, hs + 1, vs]
            else:
                chans[c] = [cw, (ch + 1) // 2, hs, vs + 1]
                res = [cw, ch - (ch + 1) // 2, hs, vs + 1]
            chans.insert(offset + (c - begin), res)
    return chans


def frame_streams(nch, w, h, squeeze=False):
    """Every (stream id, channel index within the stream, width, height) of a lossless frame as the oracle writes it: the global
    stream (id 0) holds the channels before the first one larger than a group, LF group g the later ones with shift >= 3
    (id 1 + nlf + g), pass group g the rest (id 1 + 3 nlf + kNumQuantTables + g)."""
    chans = [[w, h, 0, 0] for _ in range(nch)]
    if squeeze:
        chans = _default_squeeze(chans)
    xlf, ylf = -(-w // LF_GROUP_DIM), -(-h // LF_GROUP_DIM)
    xg, yg = -(-w // GROUP_DIM), -(-h // GROUP_DIM)
    nlf = xlf * ylf
    first = 0
    while first < len(chans) and chans[first][0] <= GROUP_DIM and chans[first][1] <= GROUP_DIM:
        first += 1
    out = [(0, c, chans[c][0], chans[c][1]) for c in range(first) if chans[c][0] and chans[c][1]]

    def group(x0, y0, dim, lo, hi, sid):
        k = 0
        for cw, ch, hs, vs in chans[first:]:
            if not cw or not ch or not lo <= min(hs, vs) <= hi:
                continue
            rw = max(0, min(dim >> hs, cw - (x0 >> hs)))
            rh = max(0, min(dim >> vs, ch - (y0 >> vs)))
            if rw and rh:
                out.append((sid, k, rw, rh))
                k += 1
    for g in range(nlf):
        group(g % xlf * LF_GROUP_DIM, g // xlf * LF_GROUP_DIM, LF_GROUP_DIM, 3, 1000, 1 + nlf + g)
    for g in range(xg * yg):
        group(g % xg * GROUP_DIM, g // xg * GROUP_DIM, GROUP_DIM, 0, 2, 1 + 3 * nlf + K_NUM_QUANT_TABLES + g)
    return out


def census(case, w, h):
    """The set of labels over every (stream, channel) of the case's frame at this size."""
    nodes = case.nodes(w, h)
    one = case.one_symbol(nodes)
    return {classify(nodes, c, sid, cw, ch, one) for sid, c, cw, ch in frame_streams(case.nch, w, h, case.squeeze)}


# ---------------------------------------------------------------- images
def picture(w, h, nch, seed, bits=8):
    from pdn_jpegxl_amd.synth import synth, synth16
    img = synth(w, h, seed) if bits == 8 else synth16(w, h, seed, bits)
    return np.ascontiguousarray({1: img[..., 1:2], 3: img[..., :3], 4: img}[nch])


def picture_of_multiples(w, h, nch, seed):
    """16-bit samples that are multiples of 384: every channel of the frame (also behind the YCoCg colour transform, which halves
    twice) then holds multiples of 96, and so does every predictor that returns a neighbour, zero or the clamped gradient."""
    img = picture(w, h, nch, seed).astype(np.uint16)
    return np.ascontiguousarray(((img * 2) // 3) * 384)   # 0 .. 170 steps of 384, the largest 65280


def picture_mixed_classes(w, h, seed):
    """RGB whose luma (channel 0 behind the colour transform) is 128 everywhere and whose two chroma channels vary."""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    co = ((xx * 3 + yy) % 41 - 20 + rng.integers(-3, 4, (h, w))).astype(np.int32)
    cg = ((xx - 2 * yy) % 37 - 18 + rng.integers(-5, 6, (h, w))).astype(np.int32)
    tmp = 128 - (cg >> 1)
    g = cg + tmp
    b = tmp - (co >> 1)
    r = b + co
    out = np.stack([r, g, b], -1)
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8))


def picture_f32(w, h, nch, seed):
    """binary32 samples, coded as their bit patterns (around 2^30): zero in the top rows and left columns, so that a channel starts
    inside the bounds of the decoder's 32-bit forms (samples below 2^18) and leaves them at its first non-zero sample."""
    img = picture(w, h, nch, seed).astype(np.float32) / 255.0
    img[h // 2:, w // 2:] *= 1e-3
    img[:h // 4] = 0
    img[:, :w // 5] = 0
    return np.ascontiguousarray(img.astype(np.float32))


# ---------------------------------------------------------------- the families
class Case:
    def __init__(self, family, name, tree, nch=1, bits=8, squeeze=False, expect=None, image=None, sizes=None, one_symbol=None, float_samples=0):
        self.family, self.name, self.nch, self.bits, self.squeeze, self.expect = family, name, nch, bits, squeeze, expect
        self.float_samples = float_samples
        self._tree, self._image, self.sizes, self._one = tree, image, sizes, one_symbol

    def nodes(self, w, h):
        return flatten(self._tree(w, h) if callable(self._tree) else self._tree)

    def one_symbol(self, nodes):
        return self._one(nodes) if self._one else ()

    def image(self, w, h):
        seed = sum(map(ord, self.name)) % 997 + w + 3 * h
        return self._image(w, h, self.nch, seed) if self._image else picture(w, h, self.nch, seed, self.bits)

    def encode_args(self):
        if self.float_samples:
            return dict(lossless=True, lossless_squeeze=self.squeeze, float_samples=self.float_samples)
        return dict(lossless=True, lossless_squeeze=self.squeeze, bits=self.bits)

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)


PLAIN = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13]
SIGNED = (8, 9, 10, 11, 12, 13, 14, 15)


def _thresholds(prop, n, rng=None):
    """n distinct sorted thresholds in the range the property takes on 8-bit pictures."""
    if prop in SIGNED:
        lo = -(n // 2)
        return list(range(lo, lo + n))
    return list(range(0, 2 * n, 2)) if prop in (4, 5, 6, 7) else list(range(n))


def random_tree(seed, with_wp, w, h):
    rng = np.random.default_rng(seed)
    props = list(range(0, 16 if with_wp else 15))
    preds = list(range(14)) if with_wp else PLAIN

    def node(depth):
        if depth == 6 or (depth > 1 and rng.random() < 0.25):
            return L(int(rng.choice(preds)), int(rng.integers(-2, 3)) if rng.random() < 0.3 else 0)
        p = int(rng.choice(props))
        if p == 0:
            v = int(rng.integers(0, 3))
        elif p == 1:
            v = int(rng.choice([0, 1, K_NUM_QUANT_TABLES + 3, K_NUM_QUANT_TABLES + 4]))
        elif p == 2:
            v = int(rng.integers(0, h + 1))
        elif p == 3:
            v = int(rng.integers(0, w + 1))
        elif p in (4, 5, 6, 7):
            v = int(rng.integers(-1, 200))
        else:
            v = int(rng.integers(-24, 25))
        return S(p, v, node(depth + 1), node(depth + 1))
    t = node(0)
    if with_wp and not uses_wp(flatten(t)):
        t = S(15, 0, t, L(6))
    return t


def _row_tree(w, h):
    cuts = sorted({0, 1, 62, 63, 64, max(h - 2, 0), h + 5})
    forms = Leaves([(0, 1, 1), (1, 0, 1), (2, -1, 1), (5, 0, 1), (1, 3, 1), (0, 0, 1), (5, -2, 1), (2, 0, 1)])
    return buckets(2, cuts, [forms() for _ in range(len(cuts) + 1)])


def _sid_tree(w, h):
    """Property 1 with a bucket of its own for every stream id of a squeezed frame: the global stream, each LF group, each pass group.
    Every bucket has another predictor, so a section decoded under a neighbour's id comes out wrong."""
    sids = sorted({sid for sid, _, _, _ in frame_streams(1, w, h, True)})
    cuts = sorted({0} | {s - 1 for s in sids if s} | {s for s in sids if s})
    leaf = Leaves([5, 1, 2, 4, 7, 8, 9, 3, 10, 11, 12, 13])
    subs = [leaf() for _ in range(len(cuts) + 1)]
    subs[-2] = S(11, 1, leaf(), leaf())     # the last pass group: a per-sample split below the static ones
    return buckets(1, cuts, subs)


def _static_tree(w, h):
    """Properties 0 and 1 above, between and below per-sample splits.  The dead children of the static nodes below hold a fourth
    and fifth property and 33 thresholds: a decoder that does not follow the live child alone leaves the grid.  (Stream ids above
    21 are the pass groups after the first of a frame with one LF group.)"""
    leaf = Leaves([5, 4, 1, 2, 7, 8, 10, 11, 12, 13, 3, 9])
    dead = lambda p: nest([(p, _thresholds(p, 33))], leaf)   # noqa: E731
    below = S(0, 5, dead(14), S(9, 3, leaf(), S(1, 21, dead(13), S(10, -1, leaf(), leaf()))))
    between = S(10, 0, S(0, 0, S(11, 2, leaf(), below), leaf()), S(1, 0, dead(12), S(11, 0, leaf(), leaf())))
    return S(0, 1, between, S(0, 0, S(1, 21, S(3, 7, leaf(), leaf()), S(3, 1, L(2), L(5, 1))), L(5)))


def _mixed_tree(w, h):
    return S(0, 1, S(10, 0, L(4), S(11, 0, L(7), L(5))), S(0, 0, S(2, 2, L(1), L(5)), L(0, 128)))


def families():
    cases = []

    def add(family, name, tree, **kw):
        cases.append(Case(family, name, tree, **kw))
    layouts = (1, 3, 4)
    # one property alone: three thresholds, the leaves cycle through the predictors
    for p in range(2, 16):
        preds = [(4 * p + i) % 14 for i in range(4)]
        preds = [q if q != 6 or p == 15 else 5 for q in preds]
        if p == 15 and 6 not in preds:
            preds[0] = 6
        thr = [-2, 0, 6] if p not in (6, 7) else [-2, 0, 100]
        add("one property", "p%d" % p, buckets(p, thr, [L(q) for q in preds]), nch=layouts[p % 3],
            expect="grid-lanes")
    # the specialised row loops
    add("specialised loops", "all 5", nest([(10, [-3, 0, 4]), (11, [-2, 2])], Leaves([5])), nch=3, expect="grid-lanes")
    add("specialised loops", "all 6 + p15", nest([(15, [-20, -3, 0, 2, 19])], Leaves([6])), nch=4, expect="grid-lanes")
    add("specialised loops", "some 6, no p15", nest([(10, [-3, 0, 4])], Leaves([6, 5, 1])), nch=1, expect="grid-lanes")
    add("specialised loops", "p15, no 6", nest([(15, [-9, 0, 8])], Leaves([5, 1, 4])), nch=3, expect="grid-lanes")
    # two slots of 32 lanes
    t32, t33 = _thresholds(10, 32), _thresholds(10, 33)
    add("layout32", "1 x 32", nest([(10, t32)], Leaves(PLAIN)), nch=1, expect="grid-lanes")
    add("layout32", "1 x 33", nest([(10, t33)], Leaves(PLAIN)), nch=3, expect="walk")
    add("layout32", "2 x 32", nest([(10, t32), (7, _thresholds(7, 32))], Leaves(PLAIN)), nch=4, expect="grid-lds")
    add("layout32", "32 + 33", nest([(11, t32), (12, _thresholds(12, 33))], Leaves(PLAIN)), nch=1, expect="walk")
    leaf = Leaves(PLAIN, 3)
    same = lambda: nest([(14, t32)], leaf)   # noqa: E731
    add("layout32", "repeated thresholds", buckets(9, [-5, 0, 0 + 5], [same(), leaf(), same(), same()]), nch=3, expect="grid-lds")
    # four slots of 16 lanes
    add("layout16", "3 props, 16", nest([(10, _thresholds(10, 16)), (3, [3, 40]), (13, [-1, 1])], Leaves(PLAIN)), nch=3, expect="grid-lds")
    add("layout16", "3 props, 17", nest([(10, _thresholds(10, 17)), (3, [3]), (13, [0])], Leaves(PLAIN)), nch=1, expect="walk")
    add("layout16", "4 props, 16", nest([(5, [10, 90]), (12, _thresholds(12, 16)), (2, [2]), (8, [0])], Leaves(PLAIN)), nch=4,
        expect="grid-lds")
    add("layout16", "4 props, 17", nest([(5, [10]), (12, [0]), (2, [2]), (8, _thresholds(8, 17))], Leaves(PLAIN)), nch=3, expect="walk")
    # grid sizes
    t3, t7, t11 = [-2, 0, 3], _thresholds(10, 7), _thresholds(10, 11)
    add("cells", "64", nest([(10, t3), (11, t3), (14, t3)], Leaves(PLAIN)), nch=1, expect="grid-lanes")
    add("cells", "65", nest([(10, _thresholds(10, 4)), (6, _thresholds(6, 12))], Leaves(PLAIN)), nch=3, expect="grid-lds")
    add("cells", "1728", nest([(9, t11), (13, t11), (11, t11)], Leaves(PLAIN)), nch=4, expect="grid-lds")
    add("cells", "2048", nest([(9, t7), (13, t7), (11, t7), (4, [4, 30, 99])], Leaves(PLAIN)), nch=1, expect="grid-lds")
    add("cells", "4096", nest([(9, t7), (13, t7), (11, t7), (12, t7)], Leaves(PLAIN)), nch=3, expect="walk")
    add("> 4 properties", "5 props", nest([(7, [60, 140]), (9, t3), (10, t3), (11, t3), (12, t3)], Leaves(PLAIN)), nch=4, expect="walk")
    # static nodes
    add("static nodes", "above between below", _static_tree, nch=4, expect="grid-lanes")
    add("static nodes", "squeezed", _static_tree, nch=3, squeeze=True, expect="grid-lanes")
    # (a channel goes to the groups only after one wider or higher than GROUP_DIM, and to an LF group only with a shift >= 3: a
    # squeezed frame needs a channel of shift 3 wider than 256, i.e. more than 2048 columns, and 33 rows for three vertical steps)
    add("static nodes", "stream ids", _sid_tree, nch=1, squeeze=True, expect="row-static", sizes=[(2100, 33)])
    add("mixed classes", "const + row + sample", _mixed_tree, nch=3, expect="const", image=lambda w, h, nch, seed: picture_mixed_classes(w, h, seed),
        one_symbol=lambda nodes: [i for i, n in enumerate(nodes) if n[0] < 0 and n[5] == 128], sizes=[(63, 5), (130, 67), (257, 70)])
    add("row trees", "rows", _row_tree, nch=3, expect="row-static", sizes=[(65, 66), (130, 67), (70, 257), (63, 5)])
    # leaf forms: multipliers and offsets (offsets of a leaf with a multiplier are multiples of it, as its residuals must be)
    rows = Leaves([(1, 1000, 2), (2, 0, 3), (5, -1000, 4), (0, 0, 96), (1, 1, 1), (0, -1, 1), (5, 999, 3), (2, 1000, 1), (1, -1, 1)])
    add("leaf forms", "row-static", lambda w, h: buckets(2, [0, 1, 2, 4, 40, 63, 64, 65], [rows() for _ in range(9)]), nch=3, bits=16,
        image=lambda w, h, nch, seed: picture_of_multiples(w, h, nch, seed), expect="row-static")
    per = Leaves([(4, 1000, 2), (7, 0, 3), (8, -1000, 4), (9, 0, 96), (5, 1, 1), (0, -1, 1), (1, 960, 96), (2, -1000, 1), (4, 1, 1)])
    add("leaf forms", "per-sample", nest([(10, [-384, 0, 383]), (3, [0, 1, 64])], per), nch=4, bits=16,
        image=lambda w, h, nch, seed: picture_of_multiples(w, h, nch, seed), expect="grid-lanes")
    # deep samples
    far = [-40001, -40000, -1, 0, 39999, 40000]
    add("deep", "no p15", nest([(9, far), (10, far), (6, [0, 40000, 65534])], Leaves(PLAIN)), nch=3, bits=16, expect="grid-lds")
    add("deep", "p15", nest([(15, far), (13, far)], Leaves(list(range(14)))), nch=1, bits=16, expect="grid-lanes")
    # float bit patterns: the 64-bit forms of the property sums and of the weighted predictor, entered inside a channel
    add("deep", "f32 no p15", nest([(8, [-2**20, 0, 2**20]), (12, [-2**22, 0, 2**22]), (3, [-1, 300]), (4, [2**29, 0x3F000000])], Leaves(PLAIN)),
        nch=3, float_samples=32, image=picture_f32, expect="grid-lds")
    add("deep", "f32 p15", nest([(15, [-2**24, -1, 0, 2**24]), (13, [-2**21, 0, 2**21]), (5, [0x3E000000, 0x3F000000])], Leaves(list(range(14)))),
        nch=1, float_samples=32, image=picture_f32, expect="grid-lanes")
    for seed in range(8):
        add("random", "plain %d" % seed, lambda w, h, s=seed: random_tree(100 + s, False, w, h), nch=layouts[seed % 3], squeeze=seed == 5)
        add("random", "weighted %d" % seed, lambda w, h, s=seed: random_tree(200 + s, True, w, h), nch=layouts[(seed + 1) % 3], squeeze=seed == 2)
    # three sizes per case, rotating so that every size occurs in every larger family
    k = 0
    for c in cases:
        if c.sizes is None:
            c.sizes = [SIZES[(k + 2 * j) % len(SIZES)] for j in range(3)]
            k += 1
    return cases


FAMILIES = ["one property", "specialised loops", "layout32", "layout16", "cells", "> 4 properties", "static nodes", "mixed classes", "row trees",
            "leaf forms", "deep", "random"]
