"""Plain Python restatement of the weight stream's schedule (fs-nerf_amd/csrc/mlp_dev.hpp, struct WStream) and of the
phase counts of a network (fs-nerf_amd/csrc/mlp_layout.hpp, build_geom): no data, only WHICH 16-KiB phase of WHICH pass
goes into WHICH ring slot and when.  The stager is mirrored member for member (begin_pass_, advance_pass_, the tail of
stage() / next_stage(), init, begin_tile, open_next); a pointer is a (pass, phase index) pair and s_left is a uint32 that
wraps like the kernel's.  The consumer side is what mlp_tile does to the stream: a tile of nph phases opens nph phases -
its own phases 1 .. nph-1 and the first phase of whatever follows (init opened the very first one)."""

K_LOOK = 2       # kLook: phases staged ahead of the one being opened
K_NSLOT = 4      # kNSlot: ring slots
K_DYNAMIC = 1 << 30  # WStream::kDynamicPhases
U32 = 0xFFFFFFFF
K_MAX_LAYERS = 16
K_AUX_CAP_FLOATS = 3456  # kAuxCapFloats

# The corner networks of the envelope (tests/test_shape_corners_gpu.py): (n_layers, d_hidden, skip, n_freqs_pos, n_freqs_dir)
CORNERS = {
    "min": (2, 128, (), 10, 4),                           # fewest phases: 3 single-pass, 6 x3
    "bare": (2, 128, (0,), 0, 0),                         # identity slots only; the one legal skip of a 2-layer net
    "deep": (16, 128, tuple(range(15)), 10, 4),           # kMaxLayers, every layer wide: the longest stream
    "wide-skips": (8, 256, tuple(range(7)), 10, 4),       # the largest aux area that fits (3392 of 3456 floats)
    "wide-min": (2, 256, (), 10, 4),                      # the shortest stream with two sample groups per wave
}


# ------------------------------------------------------------------------------------------------ build_geom
def units(n_layers, d_hidden, n_skips):
    """(units_hidden, units_total) of build_geom: 1-KiB (x3: 2-KiB) A-operand fragments, `n_skips` of the layers
    1 .. n_layers-1 fed by the position encoding as well (which ones does not change the count)."""
    assert d_hidden in (128, 256) and 2 <= n_layers <= K_MAX_LAYERS and 0 <= n_skips <= n_layers - 1
    nt = d_hidden // 32
    u = 2 * nt * 2                                   # layer 0: kKsPos = 2 encoding k-steps
    u += (n_layers - 1) * 2 * nt * nt + n_skips * 2 * nt * 2
    hidden = u
    u += 2 * nt * nt                                 # connection
    u += 2 * (nt // 2) * (nt + 1)                    # branch: kKsDir = 1
    return hidden, u


def gemms(n_layers, d_hidden, skip):
    """(output pairs, k-steps) of every GEMM in kernel order: hidden 0 .. n_layers-1, connection, branch.  Layer g > 0
    reads the encoding as well (kKsPos = 2 more k-steps) when g - 1 is in `skip`."""
    nt = d_hidden // 32
    out = [(nt, 2)]
    out += [(nt, nt + (2 if g - 1 in skip else 0)) for g in range(1, n_layers)]
    return out + [(nt, nt), (nt // 2, nt + 1)]


def kloop_shapes(n_layers, d_hidden, skip):
    """{(units per pair, offset of the pair's first unit in its 8-unit phase)} of the x3 / x2 stream: the block shapes
    gemm_layer (mlp_dev.hpp) asks kloop_block for on a 256-wide network, NU = 2 KS and OFF = (tp NU) % 8 per pair tp."""
    return {(2 * ks, (tp * 2 * ks) % 8) for npo, ks in gemms(n_layers, d_hidden, skip) for tp in range(npo)}


def phases(n_layers, d_hidden, n_skips, x3):
    """(nph_density, nph_full): 16-KiB phases of the density-only and of the full pass."""
    upp = 8 if x3 else 16
    hidden, total = units(n_layers, d_hidden, n_skips)
    assert hidden % upp == 0, "hidden units are phase aligned"
    return hidden // upp, (total + upp - 1) // upp


def aux_floats(n_layers, d_hidden):
    """build_geom's aux area: n_layers + 2 biases, the sigma head, the rgb head, 36 scalars; rounded up to 64 floats."""
    a = (n_layers + 5) * d_hidden + 36
    return (a + 63) // 64 * 64


def envelope_pairs():
    """{(nph_density, nph_full)} over n_layers 2..16 x d_hidden {128, 256} x number of skips x {single pass, x3}."""
    return sorted({phases(L, D, k, x3) for L in range(2, K_MAX_LAYERS + 1) for D in (128, 256) for k in range(L)
                   for x3 in (False, True)})


# ------------------------------------------------------------------------------------------------ WStream
class WStream:
    """`wrap_empty_tile` False: begin_tile as it was before the 3-phase fix (s_left = nph - 3 and nothing else)."""

    def __init__(self, wrap_empty_tile=True):
        self.wrap_empty_tile = wrap_empty_tile
        self.staged = []   # (pass, phase) in issue order
        self.events = []   # per opening: (slot staged into, slot opened, slot still being read, (pass, phase) opened)
        self.slots = [None] * K_NSLOT

    def begin_pass_(self, which):
        self.s_which = which
        self.s_ptr = 0  # phase index inside ptrB / ptrA
        self.s_left = self.nphB if which else self.nphA

    def advance_pass_(self):
        my_rep = self.repB if self.s_which else self.repA
        self.s_rep += 1
        if self.s_rep >= my_rep:
            self.s_rep = 0
            other = self.s_which ^ 1
            other_rep = self.repB if other else self.repA
            self.begin_pass_(other if other_rep else self.s_which)
        else:
            self.begin_pass_(self.s_which)

    def stage(self):
        self.staged.append((self.s_which, self.s_ptr))
        self.slots[self.s_slot] = (self.s_which, self.s_ptr)
        staged_into = self.s_slot
        self.s_ptr += 1
        self.s_slot = (self.s_slot + 1) % K_NSLOT
        self.s_left = (self.s_left - 1) & U32
        if self.s_left == 0:
            self.advance_pass_()
        return staged_into

    def init(self, nA, rA, nB, rB):
        self.nphA, self.repA = nA, (rA if nA else 0)
        self.nphB, self.repB = nB, (rB if nB else 0)
        self.s_rep = self.s_slot = self.c_slot = 0
        self.begin_pass_(0 if self.repA else 1)
        for _ in range(K_LOOK):
            self.stage()
        self.open_next()

    def begin_tile(self, nph):
        self.s_left = (nph - (K_LOOK + 1)) & U32
        if self.wrap_empty_tile and self.s_left == 0:
            self.advance_pass_()

    def open_next(self):
        staged_into = self.stage()
        opened = self.c_slot
        self.events.append((staged_into, opened, (opened - 1) % K_NSLOT, self.slots[opened]))
        self.c_slot = (self.c_slot + 1) % K_NSLOT


# ------------------------------------------------------------------------------------------------ consumers
def run_static(nA, rA, nB, rB, rounds, **kw):
    """render.hip: pass A (nA phases) rA times, then pass B rB times, `rounds` times over.
    -> (stream, consumed): consumed = the (pass, phase) sequence the tiles read."""
    st = WStream(**kw)
    st.init(nA, rA, nB, rB)
    consumed = []
    for _ in range(rounds):
        for which, nph, rep in ((0, nA, rA if nA else 0), (1, nB, rB if nB else 0)):
            for _ in range(rep):
                for p in range(nph):
                    consumed.append((which, p))
                    st.open_next()
    return st, consumed


def run_dynamic(tiles, **kw):
    """render_occ.hip: `tiles` = the phase counts of a run of tiles of ONE blob (pass B), each announced by begin_tile."""
    st = WStream(**kw)
    st.init(0, 0, K_DYNAMIC, 1)
    consumed = []
    for nph in tiles:
        st.begin_tile(nph)
        for p in range(nph):
            consumed.append((1, p))
            st.open_next()
    return st, consumed


def check(st, consumed, nph_of_pass, lookahead):
    """The four properties of a correct schedule; raises AssertionError naming the first that fails.
    nph_of_pass: {pass: phases of its blob}; lookahead: what the stager must have staged past the last tile."""
    want = consumed + lookahead
    assert len(st.staged) == len(consumed) + K_LOOK + 1
    for which, p in st.staged:
        assert p < nph_of_pass[which], f"phase {p} of pass {which} is past the end of its blob ({nph_of_pass[which]} phases)"
    assert st.staged == want, f"staged {st.staged[:24]} ..., consumed {want[:24]} ..."
    # every opening finds in its slot the phase the consumer reads next (events[0] is init's)
    opened = [e[3] for e in st.events]
    assert opened == want[:len(opened)], "a ring slot did not hold the phase that was opened"
    for staged_into, opened_slot, reading, _ in st.events:
        assert staged_into != opened_slot and staged_into != reading, "the stage overwrites a slot still in use"
