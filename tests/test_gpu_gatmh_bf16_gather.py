"""Option gatmh_bf16_gather (include/dorylus_hip.h): the sweep forms of the multi-head GAT gather their rows rounded to bf16
(round to nearest even) and keep every score, statistic and sum in fp32.  1 = the forward edge pass (rows of z / fg_z),
2 = and the backward's source-side pass (rows of do / bg_do).

What is pinned, stage by stage through the C-ABI (apply_vertex, apply_edge, aggregate), context A (option on) against
context B (option off):
  * forward: A equals, bit for bit, B after B's z (and fg_z) have been rounded on the host between apply_edge and aggregate;
  * backward: with gatmh_bwd_phase 1 then 2, A equals B after B's do (and bg_do) have been rounded between the phases; phase 0
    equals phase 1 followed by phase 2;
  * bf16-representable z / do: option 2 and option 0 give the same bits (nothing but the rounding differs);
  * the rounding is there (o changes) and bounded where the forward takes el from the table;
  * underflowed rows, split rows and pieces, ghost rows (two launches), overlap on / off, epoch-graph replays, learning, refusals.
Every test reads the counters gatmh_bf16_gathers_fwd / gatmh_bf16_gathers_src: the bf16 kernels really ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FWD_NAMES = ("o", "op", "m", "den", "dpos")


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def bf16(a):
    """numpy round-to-nearest-even to bf16 and back (finite values; fp32 subnormals stay bf16 subnormals)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def test_host_rounding_is_nearest_even():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, 1e-40, 1.0 + 2.0 ** -7], np.float32)
    assert np.array_equal(bf16(x), np.array([1.0, 1.0 + 2.0 ** -6, -1.0, 0.0, bf16(np.float32(1e-40)), 1.0 + 2.0 ** -7], np.float32))
    import torch
    y = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(1e-39)     # fp32 subnormals
    y = np.concatenate([y, np.random.default_rng(1).standard_normal(4096).astype(np.float32)])
    assert np.array_equal(bf16(y).view(np.uint32), torch.from_numpy(y).to(torch.bfloat16).float().numpy().view(np.uint32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def counters(ctx):
    return ctx.get_option("gatmh_bf16_gathers_fwd"), ctx.get_option("gatmh_bf16_gathers_src")


def _pad32(cols):
    return (cols + 31) // 32 * 32


def backward_takes_the_sweep_forms(K, D):
    """the dispatch of dory_aggregate(BACKWARD): gatmh_sweep_hl(K, D, ld) lanes per head, and whole heads per wave in the row-wise
    kernels ((ld / 4) % HL == 0).  A single head of at most 32 features (ld = 32: eight float4 per row, sixteen lanes per head)
    fails the second test: its forward sweeps, its backward takes the blocked kernels -- which have no bf16 form, so value 2 is
    refused for that layer and the caller runs its backward with value 1."""
    ld = _pad32(K * D)
    group = 32 if ld >= 128 else 16
    if K == 1:
        hl = 16 if (ld <= 64 and group == 16) else 0
    elif D % 4 or D & (D - 1):
        hl = 0
    else:
        hl = D // 4 if 2 <= D // 4 <= min(16, group) else 0
    return bool(hl) and (ld // 4) % hl == 0


def hub_graph(dims, V, E):
    """the graphs of tests/test_gpu_gat_mh.py::test_gat_mh_epoch_vs_oracle: random, with a hub source"""
    import partition_oracle as po
    rng = np.random.default_rng(len(dims) + V)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    s[:40], d[:40] = 3, rng.integers(0, V, 40)
    return po.preprocess(s, d, np.zeros(V, np.int64), 0, 1), rng


def make_params(rng, dims, heads, al_scale=(0.3, 0.3)):
    params = []
    for l in range(2):
        zw = dims[l + 1] * (heads[l] if l == 1 else 1)
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * al_scale[l]).astype(np.float32),
                       (rng.standard_normal(zw) * 0.3).astype(np.float32)])
    return params


def make_gatmh(da, g, dims, heads, V, X, labels, params, options=None, node_id=0, num_nodes=1, part=None, parts=None):
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V, node_id, num_nodes)
    ctx.gatmh_heads(heads)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if part is not None:
        part.upload(ctx, parts)
    else:
        ctx.graph_upload(g)
    ctx.preallocate()
    ctx.upload(0, "h", X)
    ctx.labels_upload(labels)
    for l, (W, al, ar) in enumerate(params):
        ctx.weight_set(l, "w", W)
        ctx.weight_set(l, "a_l", al)
        ctx.weight_set(l, "a_r", ar)
    return ctx


def special_rows(rng, z):
    """z with rounding ties, values next to a binade and a column of fp32 subnormals planted (finite, of the size of z)"""
    z = z.copy()
    sp = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, -0.0,
                   np.frombuffer(np.uint32(0x3FFFFFFF).tobytes(), np.float32)[0],      # 1.9999999 -> 2.0
                   np.frombuffer(np.uint32(0x3F7FFFFF).tobytes(), np.float32)[0],      # 0.99999994 -> 1.0
                   1e-40, -3e-39, 2.0 ** -133, 1.1754942e-38], np.float32)
    rows = rng.choice(z.shape[0], min(z.shape[0], 40), replace=False)
    for i, r in enumerate(rows):
        z[r, rng.integers(0, z.shape[1], 3)] = sp[(i + np.arange(3)) % sp.size]
    z[:, 1 % z.shape[1]] = (rng.uniform(0.5, 1.5, z.shape[0]) * 1e-39 * rng.choice([-1, 1], z.shape[0])).astype(np.float32)
    return z


class Pair:
    """context A (option `mode`) and context B (option 0) on the same inputs, driven stage by stage.  Ghost tensors (a rank of
    a partitioned run without a transport) are uploaded by hand from `ghosts`: {(layer, name): array}."""

    def __init__(self, da, A, B, mode, L=2, ghosts=None, plant=None, representable=False, kd=None):
        self.da, self.A, self.B, self.mode, self.L = da, A, B, mode, L
        self.kd = kd                 # [(heads, features per head)] per layer: which layers' backward takes the sweep forms
        self.src_passes = 0
        self.ghosts = ghosts or {}
        self.plant, self.representable = plant, representable
        self.o_fp32 = {}
        A.set_option("gatmh_bf16_gather", mode)
        B.set_option("gatmh_bf16_gather", 0)

    def both(self, f):
        f(self.A)
        f(self.B)

    def _ghost(self, layer, name, rounded_in_b=False, both_rounded=False):
        if (layer, name) in self.ghosts:
            a = self.ghosts[(layer, name)]
            self.A.upload(layer, name, bf16(a) if both_rounded else a)
            self.B.upload(layer, name, bf16(a) if (rounded_in_b or both_rounded) else a)

    def forward(self, compare=True, fp32_first=False):
        """every layer's forward; B's z / fg_z are rounded between apply_edge and aggregate and restored afterwards.
        fp32_first: B first aggregates the unrounded rows (kept in self.o_fp32)."""
        da = self.da
        for l in range(self.L):
            self.both(lambda c: c.apply_vertex(l, da.FORWARD))
            if self.plant is not None or self.representable:
                z = self.B.download(l, "z")
                z = self.plant(z) if self.plant is not None else z
                z = bf16(z) if self.representable else z
                self.both(lambda c: c.upload(l, "z", z))
            self._ghost(l, "fg_z", both_rounded=self.representable)
            self.both(lambda c: c.apply_edge(l + 1, da.FORWARD))
            z = self.B.download(l, "z")
            if fp32_first:
                self.B.aggregate(l + 1, da.FORWARD)
                self.o_fp32[l] = (self.B.download(l, "o"), z)
            self.B.upload(l, "z", bf16(z))
            self._ghost(l, "fg_z", rounded_in_b=True, both_rounded=self.representable)
            c0 = counters(self.A), counters(self.B)
            self.both(lambda c: c.aggregate(l + 1, da.FORWARD))
            c1 = counters(self.A), counters(self.B)
            assert c1[0][0] - c0[0][0] == (1 if self.mode >= 1 else 0) and c1[1] == c0[1] and c1[0][1] == c0[0][1], (l, c0, c1)
            self.B.upload(l, "z", z)
            self._ghost(l, "fg_z", both_rounded=self.representable)
            if compare:
                for nm in FWD_NAMES:
                    assert same_bits(self.A.download(l, nm), self.B.download(l, nm)), (l, nm)
                nxt = (l + 1, "h") if l < self.L - 1 else (l, "logits")
                assert same_bits(self.A.download(*nxt), self.B.download(*nxt)), (l, nxt)

    def backward(self, compare=True, ghost_stats=None):
        """predict, then every layer's backward in its two phases; B's do / bg_do are rounded between the phases.
        Returns A's (dz, del, gradients) per layer."""
        da = self.da
        self.both(lambda c: c.predict_gat(self.L))
        out = {}
        for l in range(self.L - 1, -1, -1):
            self.both(lambda c: c.set_option("gatmh_bwd_phase", 1))
            c0 = counters(self.A)
            swept = self.kd is None or backward_takes_the_sweep_forms(*self.kd[l])
            if not swept and self.mode >= 2:
                # this layer's backward leaves the sweep forms (see backward_takes_the_sweep_forms): refused in either phase,
                # nothing run; its backward then runs in fp32 on the unrounded rows in both contexts
                for phase in (2, 1):
                    self.A.set_option("gatmh_bwd_phase", phase)
                    with pytest.raises(da.DoryError, match="did not run the sweep form"):
                        self.A.aggregate(l + 1, da.BACKWARD)
                assert counters(self.A) == c0
                self.A.set_option("gatmh_bf16_gather", 1)
            self.both(lambda c: c.aggregate(l + 1, da.BACKWARD))
            assert counters(self.A) == c0                                    # (phase 1 gathers nothing)
            do = self.B.download(l, "do")
            if self.representable:
                do = bf16(do)
                self.both(lambda c: c.upload(l, "do", do))
            if ghost_stats is not None:
                st = self.B.download(l, "st")
                self.both(lambda c: c.upload(l, "bg_st", st[ghost_stats]))
            self._ghost(l, "bg_do", both_rounded=self.representable)
            self.B.upload(l, "do", bf16(do))
            self._ghost(l, "bg_do", rounded_in_b=True, both_rounded=self.representable)
            self.both(lambda c: c.set_option("gatmh_bwd_phase", 2))
            if not swept and self.mode >= 2:
                self.B.upload(l, "do", do)
            self.both(lambda c: c.aggregate(l + 1, da.BACKWARD))
            self.A.set_option("gatmh_bf16_gather", self.mode)
            c1 = counters(self.A)
            ran = 1 if (self.mode >= 2 and swept) else 0
            self.src_passes += ran
            assert c1[1] - c0[1] == ran and c1[0] == c0[0] and counters(self.B) == (0, 0), (l, c0, c1)
            self.B.upload(l, "do", do)
            self.both(lambda c: c.apply_vertex(l, da.BACKWARD))
            out[l] = {nm: self.A.download(l, nm) for nm in ("dz", "del")}
            out[l].update({"g_" + nm: self.A.weight_grad_get(l, nm) for nm in ("w", "a_l", "a_r")})
            if compare:
                for nm in ("dz", "del", "der", "t"):
                    assert same_bits(self.A.download(l, nm), self.B.download(l, nm)), (l, nm)
                for nm in ("a_l", "a_r", "w"):
                    assert same_bits(self.A.weight_grad_get(l, nm), self.B.weight_grad_get(l, nm)), (l, "grad", nm)
        self.both(lambda c: c.set_option("gatmh_bwd_phase", 0))
        return out

    def close(self):
        self.A.close()
        self.B.close()


SHAPES = [([40, 128, 41], [8, 1], 300, 4000),      # 8 heads x 16 on a 32-lane slab (score from the gathered row), then one head of 41 (el table)
          ([24, 32, 8], [4, 2], 200, 1500),        # 16-lane slabs, el table on both layers
          ([24, 256, 6], [4, 1], 170, 1200),       # 4 heads x 64: two 128-float slabs per row
          ([24, 256, 9], [32, 1], 140, 1000)]      # 32 heads x 8
# layers whose forward sweep takes el[u] from the table (GatFwdSweepOp::AUX_BATCH: rows narrower than 128 floats)
EL_TABLE_LAYERS = {128: (1,), 32: (0, 1), 256: (1,)}


def _pair(da, dims, heads, V, E, nb, mode, options=None, **kw):
    if nb == 0:      # the automatic layout: graphs of a few hundred vertices get no sweep layout at all (their rows fit the L2: the
        V = 20000    # fp32 path gathers row-wise there, and the option refuses -- test_refusals); one that does get it
        E = 13 * V
    kw["kd"] = [(1, dims[1]) if heads[0] == 1 else (heads[0], dims[1] // heads[0]), (heads[1], dims[2])]
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads)
    options = dict(options or {}, spmm_blk_nb=nb)
    A = make_gatmh(da, g, dims, heads, V, X, labels, params, options)
    B = make_gatmh(da, g, dims, heads, V, X, labels, params, options)
    return Pair(da, A, B, mode, **kw), rng


@pytest.mark.parametrize("nb", [0, 8])
@pytest.mark.parametrize("dims,heads,V,E", SHAPES)
def test_forward_equals_fp32_on_rounded_rows_and_rounding_is_bounded(da, dims, heads, V, E, nb):
    """tests 1 and 4 of the issue: bit equality with the fp32 path on rounded z, every layer; the rounding changes o, by at most
    2**-8 max|z| where el comes from the table (o is then a convex combination of rows rounded to 2**-9 relative; the factor two
    covers the fp32 sums)"""
    rng = np.random.default_rng(nb + dims[1])
    p, _ = _pair(da, dims, heads, V, E, nb, 1, plant=lambda z: special_rows(rng, z))
    p.forward(fp32_first=True)
    assert counters(p.A) == (2, 0) and counters(p.B) == (0, 0)
    for l in range(2):
        o_fp32, z = p.o_fp32[l]
        o_a = p.A.download(l, "o")
        assert not np.array_equal(o_a, o_fp32), l
        err, zmax = float(np.abs(o_a - o_fp32).max()), float(np.abs(z).max())
        print(f"\n{dims}/{heads} nb={nb} layer {l}: max|o_bf16 - o_fp32| = {err:.3e}, 2**-8 max|z| = {2.0 ** -8 * zmax:.3e}")
        if l in EL_TABLE_LAYERS[dims[1]]:
            assert err <= 2.0 ** -8 * zmax, (l, err, zmax)
    p.close()


@pytest.mark.parametrize("nb", [0, 8])
@pytest.mark.parametrize("dims,heads,V,E", SHAPES)
def test_backward_equals_fp32_on_rounded_rows_and_phase0_is_phase1_then_2(da, dims, heads, V, E, nb):
    p, _ = _pair(da, dims, heads, V, E, nb, 2)
    p.forward()
    phased = p.backward()
    n = p.src_passes
    assert counters(p.A) == (2, n) and n == sum(backward_takes_the_sweep_forms(*kd) for kd in p.kd) and n >= 1
    assert backward_takes_the_sweep_forms(*p.kd[0])
    # the whole backward in one call per layer (phase 0), same context: the same bits as the two phases in turn
    for l in (1, 0):
        swept = backward_takes_the_sweep_forms(*p.kd[l])
        p.A.set_option("gatmh_bf16_gather", 2 if swept else 1)
        p.A.aggregate(l + 1, da.BACKWARD)
        p.A.apply_vertex(l, da.BACKWARD)
        for nm in ("dz", "del"):
            assert same_bits(p.A.download(l, nm), phased[l][nm]), (l, nm)
        for nm in ("w", "a_l", "a_r"):
            assert same_bits(p.A.weight_grad_get(l, nm), phased[l]["g_" + nm]), (l, nm)
    assert counters(p.A) == (2, 2 * n)
    p.close()


@pytest.mark.parametrize("nb", [0, 8])
@pytest.mark.parametrize("dims,heads,V,E", SHAPES)
def test_identity_on_bf16_representable_rows(da, dims, heads, V, E, nb):
    """z and do hold bf16-representable values in both contexts: option 2 and option 0 give identical bits -- nothing but the
    rounding differs between the kernels"""
    p, _ = _pair(da, dims, heads, V, E, nb, 2, representable=True)
    p.forward()
    p.backward()
    assert counters(p.A) == (2, p.src_passes) and p.src_passes >= 1 and counters(p.B) == (0, 0)
    p.close()


@pytest.mark.parametrize("dims,heads", [([24, 64, 6], [4, 1]),        # 16-lane groups, 4 lanes per head
                                        ([40, 128, 41], [8, 1])])     # 32-lane groups, 4 lanes per head
@pytest.mark.parametrize("rows", [2, 4])
def test_forced_rows_per_group_equal_fp32_on_rounded_rows(da, dims, heads, rows):
    """option gatmh_sweep_rows 2 and 4 (tests/test_gpu_gat_mh.py: the two-row and the four-row kernels): both passes on bf16 rows
    equal the fp32 passes on host-rounded rows bit for bit"""
    p, _ = _pair(da, dims, heads, 300, 4000, 8, 2, options={"gatmh_sweep_rows": rows})
    p.forward()
    p.backward()
    assert counters(p.A) == (2, p.src_passes) and p.src_passes >= 1 and counters(p.B) == (0, 0)
    p.close()


def test_underflowed_rows_are_recomputed_from_rounded_rows(da):
    """the construction of tests/test_gpu_gat_mh.py::test_gat_mh_sweep_underflow_rows_are_recomputed: layer 0's attention vector
    scaled until most rows' denominators underflow against the upper-bound shift; the redo kernel reads rounded rows too"""
    import partition_oracle as po
    dims, heads, V, E = [40, 128, 41], [8, 1], 300, 4000
    rng = np.random.default_rng(77)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads, al_scale=(60.0, 0.3))
    A = make_gatmh(da, g, dims, heads, V, X, labels, params, {"spmm_blk_nb": 8})
    B = make_gatmh(da, g, dims, heads, V, X, labels, params, {"spmm_blk_nb": 8})
    p = Pair(da, A, B, 1)
    p.forward()
    assert counters(A) == (2, 0)
    # the premise: rows of layer 0 were recomputed -- they carry their own maximum, far below the sweep's shift
    el, er, m = A.download(0, "el").astype(np.float64), A.download(0, "er").astype(np.float64), A.download(0, "m").astype(np.float64)
    assert el.max() - el.min() > 300
    bound = el.max(0)[None, :] + er
    bound = np.where(bound > 0, bound, 0.2 * bound)
    redone = ((bound - m) > 50).any(1)
    assert redone.sum() >= 10, int(redone.sum())
    den = A.download(0, "den")
    assert np.isfinite(den).all() and (den > 0).all()
    p.close()


@pytest.mark.parametrize("dims,heads", [([40, 128, 41], [8, 1]), ([24, 32, 8], [4, 2])])
def test_split_rows_and_pieces(da, dims, heads):
    """the construction of tests/test_gpu_gat_mh.py::test_gat_mh_sweep_split_rows_and_pieces: a hub destination and a hub source
    are cut into pieces by the sweep layouts; their partial sums are combined in piece order"""
    import partition_oracle as po
    V, E = 400, 6000
    rng = np.random.default_rng(5 + len(dims) + dims[1])
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:400] = 11
    s[400:800] = 29
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    assert np.diff(g["colPtr"].astype(np.int64)).max() >= 400 and np.diff(g["rowPtr"].astype(np.int64)).max() >= 400
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads)
    A = make_gatmh(da, g, dims, heads, V, X, labels, params, {"spmm_blk_nb": 8})
    B = make_gatmh(da, g, dims, heads, V, X, labels, params, {"spmm_blk_nb": 8})
    p = Pair(da, A, B, 2)
    p.forward()
    p.backward()
    assert counters(A) == (2, 2)
    p.close()


# ---- ghost rows ---------------------------------------------------------------------------------------------------------------
def _split_inputs(P):
    """the inputs of tests/test_gpu_local_transport.py::test_local_transport_gat_mh_epoch_vs_oracle"""
    dims, heads, V, E = [40, 128, 41], [8, 1], 240, 2600
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % P).astype(np.int32)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads)
    return dims, heads, V, s.astype(np.uint32), d.astype(np.uint32), parts, X, labels, params


def test_ghost_rows_one_rank_without_transport(da):
    """rank 0 of a 2-way split in one context, ghost tensors uploaded by hand: the forward runs local-source blocks, then the
    ghost blocks (the shadow buffer's second part, converted after the wait), the source side likewise over bg_do"""
    dims, heads, V, s, d, parts, X, labels, params = _split_inputs(2)
    part = da.Partition.build(s, d, parts, 0, 2)
    g = part.view()
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    assert Gs > 0 and Gd > 0
    l2g = np.asarray(g["localToGlobal"])
    rng = np.random.default_rng(3)
    widths = [dims[1], dims[2] * heads[1]]
    ghosts = {}
    for l in range(2):
        ghosts[(l, "fg_z")] = rng.standard_normal((Gs, widths[l])).astype(np.float32)
        ghosts[(l, "bg_do")] = (rng.standard_normal((Gd, widths[l])) * 0.1).astype(np.float32)
    mk = lambda: make_gatmh(da, None, dims, heads, V, X[l2g], labels[l2g], params, {"spmm_blk_nb": 8}, 0, 2, part, parts)
    A, B = mk(), mk()
    p = Pair(da, A, B, 2, ghosts=ghosts)
    A.timing_reset()
    A.timing_enable(True)
    p.forward()
    A.sync()
    ms, n = A.timing_get("bf16_convert")
    assert n == 4, n                                      # per layer: the local rows, then the ghost rows
    # both source arrays were gathered: o depends on a ghost row and on a local row.  One launch reads one array (the launchers
    # refuse a block range that spans both), so the pass ran as two launches
    o_before = A.download(1, "o")
    bumped = dict(ghosts)
    bumped[(1, "fg_z")] = ghosts[(1, "fg_z")] + np.float32(1.0)
    A.upload(1, "fg_z", bumped[(1, "fg_z")])
    A.aggregate(2, da.FORWARD)
    assert not np.array_equal(A.download(1, "o"), o_before)
    A.upload(1, "fg_z", ghosts[(1, "fg_z")])
    A.aggregate(2, da.FORWARD)
    assert same_bits(A.download(1, "o"), o_before)
    p.backward(ghost_stats=rng.integers(0, N, Gd))
    A.sync()
    ms, n = A.timing_get("bf16_convert")
    assert n == 4 + 4 + 4, n                              # (the two repeated aggregations above, then two layers' do / bg_do)
    assert counters(A) == (4, 2)
    p.close()


@pytest.mark.parametrize("P", [2, 4])
def test_local_transport_overlap_on_and_off_give_the_same_bits(da, P):
    """P ranks over the in-process device transport, option 2, three epochs in the Engine: the ghost rows are converted only after
    their exchange has landed, so overlapping the exchange with local work changes no bit"""
    from local_ranks import run_local
    dims, heads, V, s, d, parts, X, labels, params = _split_inputs(P)
    runs, counts = [], []
    for overlap in (1, 0):
        seen = {}

        def setup(ctx, r, g):
            ctx.upload(0, "h", X[g["localToGlobal"]])
            ctx.labels_upload(labels[g["localToGlobal"]])
            for l, (W, al, ar) in enumerate(params):
                ctx.weight_set(l, "w", W)
                ctx.weight_set(l, "a_l", al)
                ctx.weight_set(l, "a_r", ar)
            close = ctx.close

            def close_and_count():                    # (run_local closes its contexts: read the counters just before)
                if r not in seen:
                    seen[r] = counters(ctx) + (int(g["srcGhostCnt"]), int(g["dstGhostCnt"]))
                close()
            ctx.close = close_and_count
        pobjs = [da.Partition.build(s, d, parts, r, P) for r in range(P)]
        dl = [(l, nm) for l in range(2) for nm in ("z", "o", "op", "t", "del", "der", "dz")] + [(1, "logits")]
        runs.append(run_local(da, pobjs, parts, dims, da.GATMH, 3, setup,
                              {"spmm_blk_nb": 8, "halo_overlap": overlap, "gatmh_bf16_gather": 2}, downloads=dl,
                              pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r")))
        counts.append(seen)
    for seen in counts:
        assert len(seen) == P
        for r, (fwd, src, Gs, Gd) in seen.items():
            assert Gs > 0 and Gd > 0 and fwd == 6 and src == 6, (r, fwd, src, Gs, Gd)     # 3 epochs x 2 layers
    a, b = runs
    for r in range(P):
        assert a["tensors"][r].keys() == b["tensors"][r].keys() and len(a["tensors"][r]) >= 15
        for k in a["tensors"][r]:
            assert same_bits(a["tensors"][r][k], b["tensors"][r][k]), (P, r, k)
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert same_bits(a["weights"][r][l][nm], b["weights"][r][l][nm]), (P, r, l, nm)
                assert same_bits(a["wgrads"][r][l][nm], b["wgrads"][r][l][nm]), (P, r, l, nm)


# ---- epoch graph, learning --------------------------------------------------------------------------------------------------
def test_replayed_epochs_are_bit_identical_to_eager(da):
    """the pattern of tests/test_gpu_epoch_graph.py, with the sweep forms forced on the small graph.  That test's multi-head
    shape ends in one head of 7 classes, a layer whose backward leaves the sweep forms (backward_takes_the_sweep_forms) and which
    value 2 therefore refuses: two heads of 8 here."""
    import partition_oracle as po
    V, E, dims, heads = 2708, 5278, [1433, 32, 8], [4, 2]
    assert not backward_takes_the_sweep_forms(1, 7) and backward_takes_the_sweep_forms(2, 8) and backward_takes_the_sweep_forms(4, 8)
    states = []
    for graph in (0, 1):
        rng = np.random.default_rng(5)
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
        g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.fill_uniform(0, "h", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(rng.integers(0, 7, V).astype(np.uint32))
        ctx.weights_init_xavier()
        ctx.adam_config(0.01)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.set_option("epoch_graph", graph)
        eng = da.NativeEngine(ctx)
        eng.run(6)
        eng.run(4)
        fwd, src = counters(ctx)
        if graph:                               # one eager epoch and one recording: replays do not count
            assert ctx.get_option("epoch_graph_recorded") == 1
            assert (fwd, src) == (4, 4), (fwd, src)
        else:
            assert (fwd, src) == (20, 20), (fwd, src)
        st = {}
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                st[(nm, l)] = ctx.weight_get(l, nm)
                st[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            for nm in ("z", "o", "op", "dz", "el", "t", "del"):
                st[(nm, l)] = ctx.download(l, nm)
        states.append(st)
        eng.close()
        ctx.close()
    for k in states[0]:
        assert same_bits(states[0][k], states[1][k]), k


def test_planted_communities_are_learned_with_bf16_rows(da):
    """the multi-head case of tests/test_gpu_learning.py (its task, its epochs, its criterion) with option 2.  That test's
    model is 4 heads x 4 features, then one head of 6 classes: the first is a shape outside gatmh_sweep_hl and the option refuses
    it (asserted here), the backward of the second leaves the sweep forms (backward_takes_the_sweep_forms).  This run takes
    4 heads x 8, then two heads of 8 logits averaged (the task's six classes use the first six), and forces the sweep layouts on
    the 6000-vertex graph (spmm_blk_nb)."""
    from test_gpu_learning import _task
    s, d, X, y, C = _task()
    V, F = X.shape
    part = da.Partition.build(s, d, np.zeros(V, np.int32), 0, 1)

    def make(hidden, C, heads):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, [F, hidden, C], V)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        part.upload(ctx)
        ctx.preallocate()
        ctx.upload(0, "h", X)
        ctx.labels_upload(y)
        ctx.weights_init_xavier()
        rng = np.random.default_rng(1)
        for l, zw in ((0, hidden), (1, C * heads[1])):
            ctx.weight_set(l, "a_l", (rng.standard_normal(zw) * 0.1).astype(np.float32))
            ctx.weight_set(l, "a_r", (rng.standard_normal(zw) * 0.1).astype(np.float32))
        ctx.adam_config(0.01)
        ctx.set_option("gatmh_bf16_gather", 2)
        return ctx
    ctx = make(16, C, [4, 1])
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    with pytest.raises(da.DoryError, match="gatmh_sweep_hl"):
        ctx.aggregate(1, da.FORWARD)
    ctx.close()
    ctx = make(32, 8, [4, 2])
    eng = da.NativeEngine(ctx)
    acc = []
    for _ in range(12):
        eng.run(5)
        logits = ctx.download(1, "logits")
        lo, hi = int(V * 0.66), int(V * 0.66) + int(V * 0.1)
        acc.append(float((logits[lo:hi].argmax(1) == y[lo:hi]).mean()))
    assert counters(ctx) == (120, 120)
    eng.close()
    ctx.close()
    print(f"\ngatmh, bf16 rows: validation accuracy {acc[0]:.3f} -> {acc[-1]:.3f}")
    assert acc[-1] > 0.85 and acc[-1] > acc[0], acc


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _usable(da, ctx, layers=(0, 1)):
    """the context still runs a forward pass in fp32 with the option back at 0"""
    ctx.set_option("gatmh_bf16_gather", 0)
    c0 = counters(ctx)
    for l in layers:
        ctx.apply_vertex(l, da.FORWARD)
        ctx.apply_edge(l + 1, da.FORWARD)
        ctx.aggregate(l + 1, da.FORWARD)
    ctx.sync()
    assert counters(ctx) == c0
    assert np.isfinite(ctx.download(layers[-1], "o")).all()


def test_refusals(da):
    for gnn in (da.GCN, da.GAT):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        for v in (1, 2):
            with pytest.raises(da.DoryError):
                ctx.set_option("gatmh_bf16_gather", v)
        ctx.set_option("gatmh_bf16_gather", 0)
        assert ctx.get_option("gatmh_bf16_gather") == 0
        ctx.close()
    ctx = da.Context(0)                       # set on a fresh context, then configured as GCN: refused there
    ctx.set_option("gatmh_bf16_gather", 1)
    with pytest.raises(da.DoryError):
        ctx.configure(da.GCN, [16, 8, 3], 100)
    ctx.close()
    ctx = da.Context(0)                       # the GCN option keeps refusing multi-head contexts
    ctx.configure(da.GATMH, [16, 8, 3], 100)
    with pytest.raises(da.DoryError):
        ctx.set_option("gcn_bf16_gather", 1)
    ctx.close()

    dims, heads, V, E = [24, 32, 8], [4, 2], 200, 1500
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads)
    ctx = make_gatmh(da, g, dims, heads, V, X, labels, params, {"spmm_blk_nb": 8})
    for bad in (3, -1):
        with pytest.raises(da.DoryError):
            ctx.set_option("gatmh_bf16_gather", bad)
        assert ctx.get_option("gatmh_bf16_gather") == 0
    with pytest.raises(da.DoryError):
        ctx.set_option("gatmh_bf16_gathers_fwd", 1)          # the counters are read-only
    # the sweep forms switched off: the blocked kernels have no bf16 form
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    ctx.set_option("gatmh_sweep", 0)
    for v in (1, 2):
        ctx.set_option("gatmh_bf16_gather", v)
        with pytest.raises(da.DoryError, match="gatmh_sweep = 0"):
            ctx.aggregate(1, da.FORWARD)
    ctx.set_option("gatmh_sweep", 1)
    # value 2, but this layer's forward ran the blocked kernels: the backward would not take the sweep forms
    ctx.set_option("gatmh_bf16_gather", 0)
    ctx.set_option("gatmh_sweep", 0)
    for l in (0, 1):
        ctx.apply_vertex(l, da.FORWARD)
        ctx.apply_edge(l + 1, da.FORWARD)
        ctx.aggregate(l + 1, da.FORWARD)
    ctx.predict_gat(2)
    ctx.set_option("gatmh_sweep", 1)
    ctx.set_option("gatmh_bf16_gather", 2)
    with pytest.raises(da.DoryError, match="forward pass did not run the sweep form"):
        ctx.aggregate(2, da.BACKWARD)
    ctx.set_option("gatmh_bf16_gather", 1)                   # (1 leaves the backward alone)
    ctx.aggregate(2, da.BACKWARD)
    # spmm_variant other than 2
    ctx.set_option("spmm_variant", 0)
    with pytest.raises(da.DoryError, match="spmm_variant"):
        ctx.aggregate(1, da.FORWARD)
    ctx.set_option("spmm_variant", 2)
    assert counters(ctx) == (0, 0)
    _usable(da, ctx)
    ctx.close()

    # no sweep layout: a graph whose rows fit the L2 gets none unless spmm_blk_nb asks for it
    dims, heads, V, E = [24, 32, 8], [4, 2], 200, 1500
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    ctx = make_gatmh(da, g, dims, heads, V, X, labels, make_params(rng, dims, heads))
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    ctx.set_option("gatmh_bf16_gather", 1)
    with pytest.raises(da.DoryError, match="sweep layout of the in-edges does not apply"):
        ctx.aggregate(1, da.FORWARD)
    assert counters(ctx) == (0, 0)
    _usable(da, ctx)
    ctx.close()

    # a shape outside gatmh_sweep_hl
    dims, heads, V, E = [12, 100, 6], [1, 1], 160, 1100
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    ctx = make_gatmh(da, g, dims, heads, V, X, labels, make_params(rng, dims, heads), {"spmm_blk_nb": 8})
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    ctx.set_option("gatmh_bf16_gather", 1)
    with pytest.raises(da.DoryError, match="gatmh_sweep_hl"):
        ctx.aggregate(1, da.FORWARD)
    assert counters(ctx) == (0, 0)
    _usable(da, ctx, layers=(0,))
    ctx.close()


def test_shadow_buffer_cannot_grow_inside_a_recording(da):
    dims, heads, V, E = [24, 32, 8], [4, 2], 200, 1500
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    ctx = make_gatmh(da, g, dims, heads, V, X, labels, make_params(rng, dims, heads), {"spmm_blk_nb": 8})
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    eng.run(1)                                               # an eager fp32 epoch: every other lazily sized buffer exists
    ctx.set_option("gatmh_bf16_gather", 2)
    ctx.epoch_graph_begin()
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    with pytest.raises(da.DoryError, match="gatmh_bf16_gather would have to grow"):
        ctx.aggregate(1, da.FORWARD)
    ctx.epoch_graph_drop()                                   # abandons the recording
    assert counters(ctx) == (0, 0)
    _usable(da, ctx)
    # after one eager epoch with the option the buffer exists, and an epoch records and replays
    ctx.set_option("gatmh_bf16_gather", 2)
    eng.run(1)
    assert counters(ctx) == (2, 2)
    ctx.set_option("epoch_graph", 1)
    eng.run(3)
    assert ctx.get_option("epoch_graph_recorded") == 1
    assert counters(ctx) == (4, 4)                           # (the recording counts, the replays do not)
    eng.close()
    ctx.close()
