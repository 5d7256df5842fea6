"""Register budget of the bf16-row multi-head GAT sweep kernels (option gatmh_bf16_gather), read from the code objects inside
the built library as tests/test_kernel_resources.py reads the fp32 ones (no GPU needed).  They run on the same one
1024-thread workgroup per CU: every instantiation stays at 128 registers or fewer, and every instantiation the launchers can
select (gatmh_sweep_rows: two rows on 16-lane launches; four on 32-lane ones, two for the source side's 16-lane heads) has no
spills -- a scratch access in the chain LDS -> gathers -> sums is a dependent miss per step."""
from test_kernel_resources import _kernels, _tparams


def test_bf16_gat_sweep_variants_fit_and_selectable_ones_do_not_spill():
    ks = _kernels()
    seen = {"fwd": set(), "src": set()}
    bad = []
    for name, (vgpr, spill) in ks.items():
        for key, stem in (("fwd", "gatmh_forward_sweep_bf16_kernel"), ("src", "gatmh_src_sweep_bf16_kernel")):
            p = _tparams(name, stem)
            if not p:
                continue
            group, hl, r, loader = p
            assert vgpr <= 128, (name, vgpr)
            cap = 2 if group == 16 else (4 if (key == "fwd" or hl != 16) else 2)
            if r <= cap:
                seen[key].add((group, hl, r))
                if spill:
                    bad.append((name, vgpr, spill))
    # every (GROUP, HL, R) the launchers select today: GROUP 16 / 32, HL 2 / 4 / 8 / 16, R 2 (and 4 on 32 lanes)
    for key in seen:
        for group in (16, 32):
            for hl in (2, 4, 8, 16):
                rows = (2,) if group == 16 or (key == "src" and hl == 16) else (2, 4)
                for r in rows:
                    assert (group, hl, r) in seen[key], (key, group, hl, r)
    assert not bad, bad


def test_bf16_gat_finish_kernels_do_not_spill():
    ks = _kernels()
    for stem in ("gatmh_forward_finish_bf16_kernel", "gatmh_forward_redo_bf16_kernel", "gatmh_src_finish_bf16_kernel"):
        names = [n for n in ks if stem in n]
        assert len(names) == 1, (stem, names)
        vgpr, spill = ks[names[0]]
        assert spill == 0, (names[0], vgpr, spill)
