"""CPU (no GPU): the weight stream's schedule (csrc/mlp_dev.hpp, WStream) restated in tests/wstream_ref.py, for every
pair of phase counts (density pass, full pass) that build_geom's envelope produces.

Two schedules exist.  The static one (render.hip: coarse density pass x repC, then fine full pass x repF, known at
init) and the dynamic one (render_occ.hip: density tiles and full tiles of one blob in an order only known while the
kernel runs, each announced by WStream::begin_tile).  For both: the phases staged, in order, are the phases consumed, in
order; no staged phase lies past the end of its blob; the slot being staged is neither the one being read nor the one
opened last; every pass has at least kLook + 1 phases.

The dynamic schedule had a defect at tiles of exactly kLook + 1 = 3 phases (a 2x128 network without skip in a
single-pass mode): begin_tile left s_left at 0, the next decrement wrapped it to 2^32 - 1 and the stager never returned
to phase 0.  test_the_model_sees_the_three_phase_defect holds the schedule as it was and shows that this model fails on
it."""
import itertools

import numpy as np
import pytest

import wstream_ref as W

PAIRS = W.envelope_pairs()
MIN_PAIR = W.phases(2, 128, 0, False)  # the only geometry with a 3-phase tile

CORNERS = W.CORNERS


def test_envelope_of_phase_counts():
    assert MIN_PAIR == (3, 7)
    assert min(d for d, _ in PAIRS) == 3 == W.K_LOOK + 1, "every pass has the kLook + 1 phases init() stages"
    assert all(d < f for d, f in PAIRS)
    three = [(L, D, k, x3) for L in range(2, 17) for D in (128, 256) for k in range(L) for x3 in (False, True)
             if W.phases(L, D, k, x3)[0] == 3]
    assert three == [(2, 128, 0, False)], "one geometry has a 3-phase density tile"
    assert W.phases(2, 128, 0, True) == (6, 13)
    assert W.K_NSLOT >= W.K_LOOK + 2


def test_aux_area_limits_256_wide_networks_to_8_layers():
    """(L + 5) d_hidden + 36 floats, rounded up to 64, must fit kAuxCapFloats = 3456."""
    assert W.aux_floats(8, 256) == 3392 <= W.K_AUX_CAP_FLOATS < W.aux_floats(9, 256)
    assert W.aux_floats(16, 128) <= W.K_AUX_CAP_FLOATS


@pytest.mark.parametrize("name", sorted(CORNERS))
@pytest.mark.parametrize("prec", [0, 1], ids=["bf16x3", "bf16"])
def test_phase_counts_against_the_packed_header(name, prec):
    """build_geom's unit count restated in wstream_ref.units == header words 8 (units), 9 (nph_full), 10 (nph_density)
    of a host-packed blob, in both unit sizes."""
    from oracle import fsnerf_oracle as O
    from test_pack_layout import pack_host
    L, D, skip, nf, nfd = CORNERS[name]
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=7)
    hw = pack_host(sd, L, D, list(skip), nf, nfd, prec)[:256].view(np.uint32)
    nd, nfull = W.phases(L, D, len(skip), prec == 0)
    assert (int(hw[8]), int(hw[9]), int(hw[10])) == (W.units(L, D, len(skip))[1], nfull, nd)
    assert int(hw[12]) == W.aux_floats(L, D)


def cyclic(nA, rA, nB, rB):
    while True:
        for which, nph, rep in ((0, nA, rA if nA else 0), (1, nB, rB if nB else 0)):
            for _ in range(rep):
                for p in range(nph):
                    yield (which, p)


@pytest.mark.parametrize("reps", [(1, 1), (2, 3), (4, 1), (1, 0), (0, 2)], ids=str)
def test_static_schedule(reps):
    """render.hip: density pass of the coarse network x repC, full pass of the fine one x repF, three rounds; (1, 0) is
    the coarse-only launch, (0, 2) a launch without a coarse pass (mlp.hip, occ_refresh.hip, train_fused.hip: one pass)."""
    rA, rB = reps
    for nd, nf in PAIRS:
        for nA, nB in ((nd, nf), (nd, nd)):
            st, consumed = W.run_static(nA, rA, nB, rB, rounds=3)
            look = list(itertools.islice(cyclic(nA, rA, nB, rB), len(consumed), len(consumed) + W.K_LOOK + 1))
            W.check(st, consumed, {0: nA, 1: nB}, look)


def test_dynamic_schedule_every_four_tiles():
    """render_occ.hip: every run of four tiles drawn from {density, full}, then the stager waits at phases 0, 1, 2."""
    look = [(1, p) for p in range(W.K_LOOK + 1)]
    for nd, nf in PAIRS:
        for kinds in itertools.product((nd, nf), repeat=4):
            st, consumed = W.run_dynamic(kinds)
            W.check(st, consumed, {1: nf}, look)


def test_dynamic_schedule_twenty_three_phase_tiles():
    nd, nf = MIN_PAIR
    look = [(1, p) for p in range(W.K_LOOK + 1)]
    for tail in ((), (nf,), (nf, nd, nf)):
        st, consumed = W.run_dynamic((nd,) * 20 + tail)
        W.check(st, consumed, {1: nf}, look)


def test_dynamic_schedule_mixed_tile_lengths():
    look = [(1, p) for p in range(W.K_LOOK + 1)]
    for tiles in itertools.product((3, 4, 6, 7, 13), repeat=4):
        st, consumed = W.run_dynamic(tiles)
        W.check(st, consumed, {1: 13}, look)


def test_the_model_sees_the_three_phase_defect():
    """begin_tile without the wrap (the code before the fix): tiles of 3, 3 and 7 phases stage phases 0 .. 12 in a row -
    past the 7 phases of the blob - instead of 0,1,2, 0,1,2, 0..6.  Tiles of four and more phases were always right."""
    st, consumed = W.run_dynamic((3, 3, 7), wrap_empty_tile=False)
    assert [p for _, p in st.staged][:13] == list(range(13))
    assert [p for _, p in consumed] == [0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 4, 5, 6]
    with pytest.raises(AssertionError, match="past the end of its blob"):
        W.check(st, consumed, {1: 7}, [(1, 0), (1, 1), (1, 2)])
    st, consumed = W.run_dynamic((3, 3, 7))
    assert [p for _, p in st.staged][:13] == [0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 4, 5, 6]
    W.check(st, consumed, {1: 7}, [(1, 0), (1, 1), (1, 2)])
    for tiles in itertools.product((4, 6, 7, 13), repeat=3):  # no 3-phase tile: the old schedule is the new one
        old, c0 = W.run_dynamic(tiles, wrap_empty_tile=False)
        new, c1 = W.run_dynamic(tiles)
        assert old.staged == new.staged and c0 == c1
