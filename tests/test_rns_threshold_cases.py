"""Holds the CPU oracle to the Python-integer restatement of rns_threshold_cases.py on inputs built to sit on every
decision threshold of the BEHZ lift and floor, scaleAndRound, plaintextTranslate and divideAndRoundQLast, at every level
of every parameter set the GPU tests (test_gpu_rns_thresholds.py) run -- and shows that every listed target is reached."""
import random

import numpy as np
import pytest

import rns_threshold_cases as cases

build_set, rows, expected_rows = cases.build_set, cases.rows, cases.expected_rows


@pytest.fixture(scope="module", params=[s[0] for s in cases.PARAMETER_SETS])
def parameter_set(request, oracle):
    return (request.param,) + build_set(oracle, request.param)


def lanes_meet_every_target(decisions, targets, lanes=4):
    return {(k % lanes, d) for k, d in enumerate(decisions)} >= {(lane, v) for lane in range(lanes) for v in targets}


def test_the_cycle_puts_every_target_on_every_lane():
    for count in (4, 6, 7, 8):
        picks = cases.cycled(count, cases.DISTINCT)
        assert lanes_meet_every_target(picks, range(count)), count


def test_lift_at_the_mtilde_threshold(parameter_set):
    name, ctx, levels = parameter_set
    for L, level in levels.items():
        tool = ctx.rns_tool(L)
        assert (level.ext[L + 1] == level.mtilde) == (L == ctx.L) and tool.bsk == level.bsk
        columns = cases.lift_threshold_columns(level, seed=100 + L)
        assert None not in columns, (name, L)
        assert lanes_meet_every_target([level.lift(x)[1] for x in columns], cases.lift_r_targets(level)), (name, L)
        assert np.array_equal(tool.lift_q_to_qbsk(rows(columns, ctx.degree)), expected_rows(columns, ctx.degree, level.lift)), (name, L)
        columns, integers = cases.lift_integer_columns(level)
        expected = expected_rows(columns, ctx.degree, level.lift)
        assert np.array_equal(tool.lift_q_to_qbsk(rows(columns, ctx.degree)), expected), (name, L)
        if L == ctx.L:
            assert cases.top_level_lift_is_centered(level, integers, [level.lift(x)[0] for x in columns]), name


def test_floor_at_the_alpha_threshold(parameter_set):
    name, ctx, levels = parameter_set
    for L, level in levels.items():
        tool = ctx.rns_tool(L)
        columns = cases.floor_threshold_columns(level, seed=200 + L)
        assert None not in columns, (name, L)
        assert lanes_meet_every_target([level.floor(x)[1] for x in columns], level.floor_alpha_targets()), (name, L)
        assert np.array_equal(tool.floor_qbsk_to_q(rows(columns, ctx.degree)), expected_rows(columns, ctx.degree, level.floor)), (name, L)
        columns = cases.floor_integer_columns(level, seed=250 + L)
        assert np.array_equal(tool.floor_qbsk_to_q(rows(columns, ctx.degree)), expected_rows(columns, ctx.degree, level.floor)), (name, L)


def test_scale_and_round_at_the_gamma_threshold(parameter_set):
    name, ctx, levels = parameter_set
    for L, level in levels.items():
        tool = ctx.rns_tool(L)
        columns = cases.scale_threshold_columns(level, seed=300 + L)
        assert None not in columns, (name, L)
        decisions = [level.scale_and_round(x)[1] for x in columns]
        if level.scale_and_round_reaches_targets():
            assert lanes_meet_every_target(decisions, level.scale_and_round_targets()), (name, L)
        else:  # Q < gamma t: the targets cannot be steered to; both sides of the comparison must still occur
            assert L == 1 and {d > level.gamma // 2 for d in decisions} == {False, True}, (name, L)
        genuine, messages = cases.scale_genuine_columns(level, seed=350 + L)
        for factor in (1, 2, level.t - 1):
            restate = lambda x: level.scale_and_round(x, factor)
            for poly in (columns, genuine):
                got = tool.scale_and_round(rows(poly, ctx.degree), factor)
                assert np.array_equal(got, expected_rows(poly, ctx.degree, restate)[0]), (name, L, factor)
            if level.noise_bound_applies():  # Delta m + v within the bound of RnsTool.swift:263 rounds to m (times the factor)
                assert [restate(x)[0] for x in genuine] == [m * factor % level.t for m in messages], (name, L, factor)


@pytest.mark.parametrize("name,t_bits", [("q40x3", 17), ("q60x8", 41), ("q60x8", 60), ("w32_27_28_28_n64", 10)])
def test_plaintext_translate_on_both_sides_of_the_fix_up(oracle, name, t_bits):
    ctx, levels = build_set(oracle, name, t_bits)
    rng = random.Random(t_bits)
    for L, level in levels.items():
        messages = cases.translate_messages(level, ctx.degree)
        shorts = [level.plaintext_translate([0] * L, m)[1] for m in messages]
        assert lanes_meet_every_target(list(zip(messages, shorts)), set(zip(messages, shorts)))
        assert {s for s in shorts} == {False, True}, (name, L)
        c0 = [[rng.randrange(qi) for qi in level.q] for _ in range(ctx.degree)]
        for polys in (2, 3):
            ct = np.zeros((1, polys, L, ctx.degree), dtype=np.uint64)
            ct[0, 0] = np.array(cases.columns_to_rows(c0), dtype=np.uint64)
            ct[0, 1:] = 7
            for subtract in (False, True):
                got = ctx.plaintext_translate(ct, np.array([messages], dtype=np.uint64), polys, subtract, moduli_count=L)
                expected = ct.copy()
                expected[0, 0] = np.array(cases.columns_to_rows(
                    [level.plaintext_translate(c, m, subtract)[0] for c, m in zip(c0, messages)]), dtype=np.uint64)
                assert np.array_equal(got, expected), (name, L, polys, subtract)


def test_mod_switch_at_the_q_last_threshold(parameter_set):
    name, ctx, levels = parameter_set
    for L in range(2, ctx.L + 1):
        moduli = levels[L].q
        columns, integers = cases.mod_switch_columns(moduli, seed=400 + L)
        decisions = [cases.divide_and_round_q_last(x, moduli)[1] for x in integers]
        assert lanes_meet_every_target(decisions, cases.q_last_remainders(moduli[-1])), (name, L)
        expected = rows([[cases.divide_and_round_q_last(x, moduli)[0] % m for m in moduli[:-1]] for x in integers], ctx.degree)
        data = rows(columns, ctx.degree)
        assert np.array_equal(ctx.ciphertext_context(L).divide_and_round_q_last(data)[0], expected), (name, L)
        ct = np.stack([data, data[:, ::-1]])[None]
        got = ctx.mod_switch_down(ct, 2, L)
        assert np.array_equal(got[0, 0], expected) and np.array_equal(got[0, 1], expected[:, ::-1]), (name, L)
        # the chain to one modulus: every step's remainder on a listed value
        columns, integers = cases.mod_switch_chain_columns(moduli, seed=450 + L)
        finals = [cases.mod_switch_chain(x, moduli) for x in integers]
        for step in range(L - 1):
            assert {f[1][step] for f in finals} == set(cases.q_last_remainders(moduli[L - 1 - step])), (name, L, step)
        chain = rows(columns, ctx.degree)[None, None]
        for count in range(L, 1, -1):
            chain = ctx.mod_switch_down(chain, 1, count)
        assert np.array_equal(chain[0, 0], rows([[f[0] % moduli[0]] for f in finals], ctx.degree)), (name, L)


def test_the_sets_take_every_kernel_form(oracle):
    """The two host flags that choose the lift / floor kernel forms: both values of wide_reduce_ok among the 8-byte sets, and
    the bounded (wide_reduce_ok) lift both with two coefficients per lane (L <= 6) and with one (L > 6)."""
    wide, merge, wide_moduli_counts = set(), set(), set()
    # floor_merge_ok = 0 needs (L + 2) (Bsk - 1) (q - 1) >= 2^127; Bsk primes sit just above 2^60 and q < 2^62, so their product is
    # about 2^122 and L would have to pass 30 -- the kernels stop at 16 moduli.  No parameter set reaches the separate
    # correction of floor_kernel, so only the merged one can be asked for here.
    for name, word_bits, *_ in cases.PARAMETER_SETS:
        if word_bits == 64:
            for L, level in build_set(oracle, name)[1].items():
                wide.add(cases.wide_reduce_ok(level))
                merge.add(cases.floor_merge_ok(level))
                if cases.wide_reduce_ok(level):
                    wide_moduli_counts.add(L <= 6)
    assert wide == {False, True} and merge == {True} and wide_moduli_counts == {False, True}
