"""The value-domain check of the hand-scheduled trunk body (tools/h3asm/gen.py: every epilogue unit's v_max3 reduction and
compare, the tile's one exec-masked global_atomic_or) run in the functional simulator (tools/h3asm/check.py) on one 128-point
tile: activations beyond the fp16 range set the build's bit (NSFF_RANGE_ACT for inference, NSFF_RANGE_SAVED for the training
forward's SAVE build) exactly once, the same tile in range leaves the word at zero, and the stream stays hazard-free."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "h3asm"))
import check  # noqa: E402
import gen  # noqa: E402
import isa  # noqa: E402

ACT, SAVED = 0x1, 0x2


@pytest.mark.parametrize("kind,bit", [("static", ACT), ("static_save", SAVED), ("dynamic_tb", ACT)])
def test_out_of_range_activation_sets_the_bit(kind, bit):
    assert check.run_case(kind, verbose=False, poke=1.0e5) == bit


@pytest.mark.parametrize("kind", ["static", "static_save"])
def test_in_range_tile_leaves_the_word_zero(kind):
    assert check.run_case(kind, verbose=False, poke=0.05) == 0


def test_the_check_is_in_every_epilogue_unit_and_the_lint_is_clean():
    for save in (False, True):
        pre, prog, bodies = gen.build(save=save)
        assert gen.lint(bodies, prog) == []
        ops = [i.op for i in prog]
        assert ops.count("gatomic_or_s") == 1
        for name, ins in bodies.items():         # every epilogue stream (64 values a lane): 32 v_max3, one compare
            relu = sum(1 for i in ins if i.op == "v_max_f32" and i.args["s"][0] == 0)
            assert sum(1 for i in ins if i.op == "v_max3_f32") * 2 == relu, name
            assert sum(1 for i in ins if i.op == "v_cmp_nge_f32") * 64 == relu, name
        tail = prog[[i.op for i in prog].index("gatomic_or_s") - 8:]
        assert any(i.op == "s_mov_exec" for i in tail)


def test_simulated_instructions():
    """v_max3_f32 drops a NaN operand, v_cmp_nge_f32 counts NaN as out of range, s_or_b64 / s_cmp_lg_u64 see all 64 bits"""
    sim = isa.Sim([isa.I_v_max3(isa.V(3), isa.V(0), isa.V(1), isa.V(2)),
                   isa.I_v_cmp_nge_f32_s(isa.S(10, 2), isa.S(4), isa.V(3)),
                   isa.I_v_cmp_nge_f32_s(isa.S(12, 2), isa.S(4), isa.V(2)),
                   isa.I_salu("s_or_b64", isa.S(14, 2), isa.S(10, 2), isa.S(12, 2), scc=True),
                   isa.I_s_cmp("s_cmp_lg_u64", isa.S(14, 2), 0)])
    w = sim.waves[0]
    v0 = np.zeros(64, np.float32); v0[40] = 7e4
    v2 = np.zeros(64, np.float32); v2[1] = np.nan
    w.v[0], w.v[1], w.v[2] = v0.view(np.uint32), np.zeros(64, np.uint32), v2.view(np.uint32)
    w.s[4] = np.float32(65504.0).view(np.uint32)
    for _ in range(5):
        sim.step(w)
    m = w.v[3].view(np.float32)
    assert m[40] == 7e4 and m[1] == 0.0
    bits = int(w.s[14]) | (int(w.s[15]) << 32)
    assert bits == (1 << 40) | (1 << 1) and w.scc == 1
