"""The case table of the entropy-code forms (tests/test_entropy_forms.py on the CPU, tests/test_gpu_entropy_forms.py on the GPU): streams
written with oracle_lib.encode(entropy=...), i.e. hybrid-integer configurations other than (4, 2, 0), LZ77 with every special distance,
plain distances, other thresholds and length codes, and the ANS histogram forms the writer does not choose on its own.

A case names what it is built to reach as a predicate on oracle_lib.entropy_census(); a case whose predicate fails is an error."""
import numpy as np

from pdn_jpegxl_amd.synth import synth

# the format's table of special distances, (dx, dy) by index (ISO/IEC 18181-1, C.3.3), written out here from its definition
SPECIAL = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3),
           (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3),
           (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5),
           (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1),
           (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7),
           (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
           (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6),
           (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]

ZERO_TREE = [[-1, 0, 0, 0, 0, 0, 1]]        # one leaf, the Zero predictor: the tokens are the samples themselves
ALL_SPECIAL = list(range(120))


def row_tree(h):
    """A leaf per row (property 2), predictors 0 / 1 / 2 / 5 in turn: every channel is row-static (scalar rows, RowScalar)."""
    import ma_tree_util as M
    return M.flatten(M.buckets(2, list(range(h - 1)), [M.L((0, 1, 2, 5)[y % 4]) for y in range(h)]))


def grid_tree():
    """Thresholds on a per-sample property (10: W - NW), predictors 5 / 4 / 7: the uniform-shape decoder with its grid in lanes."""
    import ma_tree_util as M
    return M.flatten(M.buckets(10, [-30, -9, -2, 0, 3, 11, 40], [M.L(p) for p in (5, 4, 7, 5, 4, 7, 5, 4)]))


def many_leaves_tree():
    """81 leaves on property 10: with wide_codes more than eight clusters, so the context map is not written in its simple form."""
    import ma_tree_util as M
    return M.flatten(M.buckets(10, [3 * (k - 40) for k in range(80)], [M.L((5, 4, 7, 1)[k % 4]) for k in range(81)]))


TREES = {"default": lambda h: None, "rows": row_tree, "grid": lambda h: grid_tree(), "zero": lambda h: ZERO_TREE, "many": lambda h: many_leaves_tree()}


# ---------------------------------------------------------------- pictures
def noise(w, h, nch, seed, hi=256, dtype=np.uint8):
    return np.random.default_rng(seed).integers(0, hi, (h, w, nch)).astype(dtype)


def graded(w, h, nch, seed):
    """Noise whose amplitude doubles from row to row (1 .. 128 and again): rows, hence contexts, with different token statistics."""
    rng = np.random.default_rng(seed)
    amp = (1 << (np.arange(h) % 8))[:, None, None]
    return (rng.integers(0, 256, (h, w, nch)) % (2 * amp)).astype(np.uint8)


def banded(w, h, pairs, seed):
    """Gray picture of bands, one per (dx, dy): dy rows of noise, then one row whose sample x repeats (x - dx, y - dy) where that lies
    inside the row and is noise elsewhere (dy = 0: a row of period dx).  Under the Zero predictor the row holds one match of w - |dx|
    values at exactly that offset; rows below the bands are noise."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (h, w), dtype=np.uint8)
    y = 0
    for dx, dy in pairs:
        y += dy
        assert y < h, "bands do not fit"
        for x in range(w):
            if 0 <= x - dx < w and (dy or dx):
                px[y, x] = px[y - dy, x - dx]
        y += 1
    return px[:, :, None]


def pack_bands(indices, h):
    """Special indices -> lists whose bands (dy + 1 rows each) fit h rows, first fit over decreasing dy."""
    files = []
    for k in sorted(indices, key=lambda k: (-SPECIAL[k][1], k)):
        need = SPECIAL[k][1] + 1
        for f in files:
            if f[0] + need <= h:
                f[0] += need
                f[1].append(k)
                break
        else:
            files.append([need, [k]])
    return [f[1] for f in files]


def periodic(w, h, periods, seed):
    """Gray picture whose samples, in raster order, repeat with the given periods, a stretch each (plain distances, rows ignored)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, w * h, dtype=np.uint8)
    n = w * h // len(periods)
    for j, p in enumerate(periods):
        for i in range(j * n + p, (j + 1) * n):
            v[i] = v[i - p]
    return v.reshape(h, w, 1)


def runs(w, h, length, seed):
    v = np.repeat(np.random.default_rng(seed).integers(0, 256, -(-w * h // length), dtype=np.uint8), length)[:w * h]
    return v.reshape(h, w, 1)


def equal_tokens16(w, h):
    """Sixteen sample values, equally often (w * h a multiple of 16), one for each of the tokens 16 .. 31 of configuration (4, 2, 0)
    under the Zero predictor (the value coded for sample v is 2 v): fifteen zero counts, the omitted count, then fifteen equal counts, so
    the last run-length symbol runs to the alphabet's end."""
    assert (w * h) % 16 == 0
    vals = np.array([8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112], np.uint8)
    v = np.tile(vals, w * h // 16)
    return np.random.default_rng(5).permutation(v).reshape(h, w, 1)


def tiles_rgba(wb, hb, ids, seed):
    """RGBA picture of 8 x 8 tiles: tile (bx, by) is noise keyed by ids[by, bx], so equal ids give equal LF values (and equal blocks)."""
    rng = np.random.default_rng(seed)
    bank = {}
    px = np.zeros((hb * 8, wb * 8, 4), np.uint8)
    for by in range(hb):
        for bx in range(wb):
            k = int(ids[by, bx])
            if k not in bank:
                base = rng.integers(30, 226, 3)
                bank[k] = np.clip(base + rng.integers(-24, 25, (8, 8, 3)), 0, 255).astype(np.uint8)
            px[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8, :3] = bank[k]
    px[..., 3] = 255
    return px


def lossy_lz_picture(w, h, lf_pairs, alpha_pairs, seed):
    """w x h RGBA: the LF image repeats itself at lf_pairs band by band, alpha at alpha_pairs."""
    wb, hb = -(-w // 8), -(-h // 8)
    ids = banded(wb, hb, lf_pairs, seed)[..., 0].astype(np.int64)
    # (banded() draws bytes: distinct noise cells may share an id, which only adds matches)
    px = tiles_rgba(wb, hb, ids, seed + 1)[:h, :w].copy()
    # below the bands: the same smooth tile over and over (a ramp across each block), whose few coefficients give the HF stream a short
    # period - copies there run on over many blocks, across each block's last coefficient into the next one's non-zero counts
    y0 = 8 * sum(dy + 1 for _, dy in lf_pairs)
    assert y0 + 24 <= h
    px[y0:, :, :3] = (90 + 12 * (np.arange(w) % 8))[None, :, None]
    px[..., 3] = banded(w, h, alpha_pairs, seed + 2)[..., 0]
    return px


def zero_start_rgba(w, h, seed):
    px = synth(w, h, seed)
    px[:16] = 0   # black and transparent: LF, HF non-zero counts and alpha all begin with zeros
    return px


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, group, name, picture, entropy, check, lossless=True, enc=None, tree=None, plan=None):
        self.group, self.name, self.picture, self.entropy, self.check = group, name, picture, entropy, check
        self.lossless, self.enc, self.tree, self.plan = lossless, dict(enc or {}), tree, dict(plan or {})

    def args(self):
        """Keyword arguments of encode() without entropy=."""
        a = dict(self.enc)
        if self.lossless:
            a["lossless"] = True
            if self.tree is not None:
                h = self.picture().shape[0]
                t = TREES[self.tree](h)
                if t is not None:
                    a["tree"] = t
        else:
            a.setdefault("distance", 1.0)
        return a

    def encode(self, oracle, entropy=True):
        return oracle.encode(self.picture(), entropy=self.entropy if entropy else None, **self.args())

    @property
    def id(self):
        return "%s/%s" % (self.group, self.name)


def data_codes(cen):
    """The census entries of the codes that carry samples or coefficients (not the MA tree's own code, which has six contexts)."""
    return [c for c in cen["codes"] if c["contexts"] != 6]


def uses(*cfgs):
    want = {tuple(c) for c in cfgs}

    def check(cen):
        seen = {tuple(g) for c in data_codes(cen) for g in c["cfgs"]}
        assert want <= seen, (want, seen)
    return check


def mixed(n):
    def check(cen):
        assert any(len({tuple(g) for g in c["cfgs"]}) >= n for c in data_codes(cen)), [c["cfgs"] for c in data_codes(cen)]
    return check


def both(*checks):
    def check(cen):
        for c in checks:
            c(cen)
    return check


def tail_bits(n):
    def check(cen):
        assert cen["max_tail_bits"] >= n, cen["max_tail_bits"]
    return check


def specials(indices):
    def check(cen):
        missing = [k for k in indices if not cen["special"][k]]
        assert not missing, "special distances never written: %s" % missing
    return check


def census_has(**least):
    def check(cen):
        for k, v in least.items():
            assert cen[k] >= v, (k, cen[k], v)
    return check


def every_data_code(**least):
    def check(cen):
        for c in data_codes(cen):
            for k, v in least.items():
                assert c[k] >= v, (k, c[k], v, c["contexts"])
    return check


def hf_code(**least):
    def check(cen):
        hf = [c for c in cen["codes"] if c["contexts"] >= 495]
        assert hf
        for k, v in least.items():
            assert all(c[k] >= v for c in hf), (k, [c[k] for c in hf], v)
    return check


def hf_small_distances(cen):
    hf = [c for c in cen["codes"] if c["contexts"] >= 495]
    assert hf and all(min(c["general_small"][1:4]) >= 1 and c["overlapping"] >= 3 and c["longest_copy"] > 195 for c in hf), \
        [(c["general_small"], c["overlapping"], c["longest_copy"]) for c in hf]


def split_is_log_alpha(cen):
    assert all(c["log_alpha"] == g[0] for c in cen["codes"] for g in c["cfgs"]), [(c["log_alpha"], c["cfgs"]) for c in cen["codes"]]


def shift_written(s):
    def check(cen):
        assert cen["hist_shift"].get(s, 0) >= 1, cen["hist_shift"]
    return check


MIXED5 = [(4, 2, 0), (0, 0, 0), (4, 0, 4), (4, 4, 0), (4, 1, 1)]
MIXED_WIDE = [(5, 2, 1), (4, 1, 1), (6, 3, 2), (8, 0, 0)]


def _cfg_cases():
    out = []
    rgb = lambda: noise(33, 17, 3, 11)             # noqa: E731
    rgb40 = lambda: graded(40, 24, 3, 12)          # noqa: E731
    g16 = lambda: noise(40, 24, 1, 13, 65536, np.uint16)   # noqa: E731
    small = lambda: noise(40, 24, 1, 14, 16)       # noqa: E731
    six = lambda: graded(33, 17, 3, 15) >> 2       # noqa: E731
    above = lambda: (64 + noise(33, 17, 1, 16, 16))   # noqa: E731
    for tree in ("default", "rows", "grid"):
        out.append(Case("cfg", "000 16-bit noise %s" % tree, g16, dict(cfgs=[(0, 0, 0)]), both(uses((0, 0, 0)), tail_bits(16)), enc=dict(bits=16), tree=tree))
        for cfg in ((4, 0, 4), (4, 4, 0), (4, 1, 1)):
            out.append(Case("cfg", "%d%d%d %s" % (cfg + (tree,)), rgb, dict(cfgs=[cfg]), uses(cfg), tree=tree))
        out.append(Case("cfg", "521 wide %s" % tree, rgb, dict(cfgs=[(5, 2, 1)]), uses((5, 2, 1)), enc=dict(wide_codes=True), tree=tree))
        out.append(Case("cfg", "632 prefix %s" % tree, rgb, dict(cfgs=[(6, 3, 2)]), uses((6, 3, 2)), enc=dict(prefix_codes=True), tree=tree))
        out.append(Case("cfg", "mixed %s" % tree, rgb40, dict(cfgs=MIXED5), mixed(3), tree=tree))
        out.append(Case("cfg", "mixed wide %s" % tree, six, dict(cfgs=MIXED_WIDE), mixed(3), enc=dict(wide_codes=True), tree=tree))
    # values that fit: every token below 1 << log_alpha although nothing is ever read behind a token
    out.append(Case("cfg", "800 wide fits", six, dict(cfgs=[(8, 0, 0)]), uses((8, 0, 0)), enc=dict(wide_codes=True, transforms=[]), tree="zero"))
    out.append(Case("cfg", "500 split = log_alpha", small, dict(cfgs=[(5, 0, 0)]), both(uses((5, 0, 0)), split_is_log_alpha), tree="zero"))
    # one symbol in the cluster, at or above the split: no ANS bits, but six tail bits a sample (under (4, 1, 0) the values 2 * 64 .. 2 * 79 share token 22)
    out.append(Case("cfg", "one symbol above the split", above, dict(cfgs=[(4, 1, 0)]), both(every_data_code(hist_simple=1), tail_bits(6)), tree="zero"))
    out.append(Case("cfg", "mixed wide many leaves", rgb40, dict(cfgs=MIXED_WIDE[:3]), mixed(3), enc=dict(wide_codes=True), tree="many",
                    plan=dict(mod_global=1)))
    out.append(Case("cfg", "1x64 000", lambda: noise(1, 64, 1, 17), dict(cfgs=[(0, 0, 0)]), uses((0, 0, 0)), tree="default"))
    return out


# lossy frames: 64 x 64 (one group) and 264 x 264 (two groups across), RGBA
def _lossy(w, seed):
    return lambda: synth(w, w, seed)


def _lossy_cfg_cases():
    out = []
    for w in (64, 264):
        p = _lossy(w, 20 + w)
        out.append(Case("cfg-lossy", "404 %d" % w, p, dict(cfgs=[(4, 0, 4)]), uses((4, 0, 4)), lossless=False))
        out.append(Case("cfg-lossy", "411 %d" % w, p, dict(cfgs=[(4, 1, 1)]), uses((4, 1, 1)), lossless=False))
        out.append(Case("cfg-lossy", "mixed %d" % w, p, dict(cfgs=MIXED5), mixed(4), lossless=False))
        out.append(Case("cfg-lossy", "632 prefix %d" % w, p, dict(cfgs=[(6, 3, 2)]), uses((6, 3, 2)), lossless=False, enc=dict(prefix_codes=True)))
        out.append(Case("cfg-lossy", "mixed wide %d" % w, p, dict(cfgs=MIXED_WIDE[:3]), mixed(3), lossless=False, enc=dict(wide_codes=True),
                        plan=dict(hf_global=1) if w == 264 else None))
    # 81 leaves on the alpha and LF trees, kept apart by wide codes: the tables of lf_ans_kernel and alpha_ans_kernel leave LDS too
    many = many_leaves_tree()
    out.append(Case("cfg-lossy", "mixed wide many leaves 264", _lossy(264, 284), dict(cfgs=MIXED_WIDE[:3]), mixed(3), lossless=False,
                    enc=dict(wide_codes=True, alpha_tree=many, lf_tree=many), plan=dict(hf_global=1, lf_global=1, alpha_global=1)))
    return out


SPECIAL_FILES = pack_bands(ALL_SPECIAL, 24)
LF_PAIRS = [3, 119, 77, 91, 117]        # (-1, 1), (8, 7), (-5, 5), (-7, 3), (-7, 7)
ALPHA_PAIRS = [79, 89, 112, 9, 98, 23]  # (-7, 1), (-3, 7), (-6, 7), (-2, 1), (-4, 7), (4, 0)


def _lz_cases():
    out = []
    allsp = dict(distances=ALL_SPECIAL)
    for i, ks in enumerate(SPECIAL_FILES):
        out.append(Case("lz-special", "file %02d" % i, (lambda ks=ks, i=i: banded(40, 24, [SPECIAL[k] for k in ks], 100 + i)), dict(lz=allsp),
                        specials(ks), tree="zero"))
    # offsets below 1: width 1, (-1, 1) and (-2, 1) -> 0 and -1; width 2, (-2, 1) and (-3, 1) -> 0 and -1
    for w, ks in ((1, [3]), (1, [9]), (2, [9]), (2, [17])):
        out.append(Case("lz-clamp", "%dx64 index %d" % (w, ks[0]), (lambda w=w: runs(w, 64, 7, 130 + w)), dict(lz=dict(distances=ks)),
                        both(specials(ks), census_has(overlapping=3)), tree="zero"))
    # a palette of 24 colours over an 8-wide picture: the meta channel (24 x 3) is the widest of the section
    out.append(Case("lz-misc", "palette wider than the picture", lambda: _palette_picture(), dict(lz=allsp), census_has(longest_copy=3),
                    enc=dict(palette=True)))
    per = lambda: periodic(40, 24, [13, 37, 5], 140)   # noqa: E731
    gen = dict(distances=["general"])
    out.append(Case("lz-misc", "general distances", per, dict(lz=gen), census_has(general=3, general_max=37), tree="zero"))
    out.append(Case("lz-misc", "general, distance tail", per, dict(lz=gen, cfgs=[(0, 0, 0)]), census_has(general=3, max_dist_tail_bits=7), tree="zero"))
    out.append(Case("lz-misc", "overshoot", per, dict(lz=dict(gen, overshoot=True)), census_has(clamped=1), tree="zero"))
    out.append(Case("lz-misc", "min_symbol 225", per, dict(lz=dict(gen, min_symbol=225, max_len=40)), census_has(general=3), tree="zero"))
    out.append(Case("lz-misc", "min_symbol 512 prefix", per, dict(lz=dict(gen, min_symbol=512)), census_has(general=3), tree="zero", enc=dict(prefix_codes=True)))
    for ml in (4, 9, 40):
        out.append(Case("lz-misc", "min_length %d" % ml, per, dict(lz=dict(gen, min_length=ml)), census_has(general=2), tree="zero"))
    out.append(Case("lz-misc", "len_cfg 000, 1000+", lambda: runs(40, 48, 1200, 141), dict(lz=dict(gen, len_cfg=(0, 0, 0), max_len=2000)),
                    census_has(longest_copy=1000, max_tail_bits=10), tree="zero"))
    out.append(Case("lz-misc", "len_cfg 800", per, dict(lz=dict(gen, len_cfg=(8, 0, 0), max_len=30)), census_has(general=3), tree="zero"))
    out.append(Case("lz-misc", "len_cfg 800 prefix, 1000+", lambda: runs(40, 48, 1200, 142), dict(lz=dict(gen, len_cfg=(8, 0, 0), max_len=2000)),
                    census_has(longest_copy=1000), tree="zero", enc=dict(prefix_codes=True)))
    zs = lambda: np.concatenate([np.zeros((3, 40, 1), np.uint8), noise(40, 21, 1, 143)])   # noqa: E731
    out.append(Case("lz-zero-start", "lossless", zs, dict(lz=dict(zero_start=True)), census_has(zero_start=1), tree="zero"))
    out.append(Case("lz-zero-start", "lossless prefix", zs, dict(lz=dict(zero_start=True)), census_has(zero_start=1), tree="zero", enc=dict(prefix_codes=True)))
    # lossy frames: special distances on the LF image (33 x 33) and on alpha, plain ones everywhere, short periods on the HF stream
    pic = lambda: lossy_lz_picture(264, 264, [SPECIAL[k] for k in LF_PAIRS], [SPECIAL[k] for k in ALPHA_PAIRS], 150)   # noqa: E731
    zero_trees = dict(alpha_tree=ZERO_TREE, lf_tree=ZERO_TREE, gaborish=False)
    out.append(Case("lz-lossy", "special 264", pic, dict(lz=allsp), specials(LF_PAIRS + ALPHA_PAIRS), lossless=False, enc=zero_trees))
    out.append(Case("lz-lossy", "general 264", pic, dict(lz=dict(distances=["general"], len_cfg=(0, 0, 0), max_len=2000)),
                    both(every_data_code(general=1), hf_small_distances), lossless=False, enc=zero_trees))
    out.append(Case("lz-lossy", "general 64", _lossy(64, 151), dict(lz=dict(distances=["general"], general_max=3)),
                    every_data_code(general=1), lossless=False))
    out.append(Case("lz-zero-start", "lossy 264", lambda: zero_start_rgba(264, 264, 152), dict(lz=dict(zero_start=True)),
                    every_data_code(zero_start=1), lossless=False, enc=zero_trees))
    return out


def _palette_picture():
    rng = np.random.default_rng(160)
    colours = rng.integers(0, 256, (24, 3), dtype=np.uint8)
    idx = np.repeat(rng.integers(0, 24, (24, 2)), 4, axis=1)   # runs of four along each row of 8
    return colours[idx]


def _hist_cases():
    out = []
    rgb = lambda: noise(40, 24, 3, 170)   # noqa: E731
    lossy = _lossy(64, 171)
    forms = [("flat", "flat", census_has(hist_flat=1, hist_flat_not_pow2=1))]
    forms += [("shift %d" % s, ("shift", s), shift_written(s)) for s in (0, 5, 12)]
    forms += [("rle", "rle", census_has(hist_rle=1))]
    for name, form, check in forms:
        out.append(Case("hist", name + " lossless", rgb, dict(hist=form), check, tree="default"))
        out.append(Case("hist", name + " lossy", lossy, dict(hist=form), check, lossless=False))
    out.append(Case("hist", "rle to the alphabet's end", lambda: equal_tokens16(40, 24), dict(hist="rle"), census_has(rle_to_end=1), tree="zero"))
    out.append(Case("hist", "mtf lossy", lossy, dict(ctx_map_mtf=True), census_has(mtf_maps=1, mtf_largest=65), lossless=False))
    out.append(Case("hist", "mtf lossless wide", rgb, dict(ctx_map_mtf=True), census_has(mtf_maps=1, mtf_largest=65), enc=dict(wide_codes=True), tree="many",
                    plan=dict(mod_global=1)))
    return out


CASES = _cfg_cases() + _lossy_cfg_cases() + _lz_cases() + _hist_cases()
assert len({c.id for c in CASES}) == len(CASES)


def cases_of(*groups):
    return [c for c in CASES if c.group in groups]


# (name, entropy, encode options): headers no decoder may accept
REFUSALS = [("msb > split", dict(bad_cfg=(4, 5, 0)), {}),
            ("lsb + msb > split", dict(bad_cfg=(4, 2, 3)), {}),
            ("split > log_alpha", dict(bad_cfg=(6, 0, 0)), {}),
            ("shift > 13", dict(bad_hist="shift14"), {}),
            ("run-length symbol after the omitted position", dict(bad_hist="rle_after_omit"), {})]


# ---------------------------------------------------------------- corrupt variants of one LZ77 stream
def corrupt_variants(oracle):
    """One 40 x 24 frame (a bare codestream of one section, so the section is the file's tail) whose first copy reads extra bits for its
    length and for its distance; the census says where.  Returns (source, file, [(name, damaged file)]): single flipped bits in the
    length's extra bits and in the distance's, and the stream cut short.  Extra bits do not touch the ANS state, so not every flip is
    an error: what each variant decodes to - an error or pixels - is the oracle's to say, and the product's to repeat."""
    src = periodic(40, 24, [13, 37, 5], 140)
    data = oracle.encode(src, lossless=True, tree=ZERO_TREE, container=False,
                         entropy=dict(cfgs=[(0, 0, 0)], lz=dict(distances=["general"], len_cfg=(0, 0, 0))))
    code = oracle.entropy_census()["codes"][-1]
    assert code["first_len_tail_bit"] >= 0 and code["first_dist_tail_bit"] > code["first_len_tail_bit"]
    section = -(-code["first_end_bit"] // 8)

    def flip(bit):
        b = 8 * (len(data) - section) + bit
        out = bytearray(data)
        out[b >> 3] ^= 1 << (b & 7)
        return bytes(out)
    variants = [("length bit 0", flip(code["first_len_tail_bit"])), ("length bit 1", flip(code["first_len_tail_bit"] + 1)),
                ("distance bit 0", flip(code["first_dist_tail_bit"])), ("distance bit 2", flip(code["first_dist_tail_bit"] + 2)),
                ("truncated", data[:-section // 2])]
    return src, data, variants
