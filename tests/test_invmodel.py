"""CPU tests of tests/invmodel.py, the model tests/test_gpu_inverse_limits.py holds the GPU inverse to: against the
oracle's forward and inverse transforms on every block that file uses, against the goldens of the reference, and
on damaged input, where the oracle's walk and the model must refuse the same inputs."""
import base64
import json
import os

import numpy as np
import pytest

import invmodel

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = invmodel.SIZES[-1]
PARAMS = [(s, tuple(invmodel.block_names(s))) for s in invmodel.SIZES[:-1]] + [(BIG, (k,)) for k in invmodel.block_names(BIG)]


def _ids(p):
    return "%d-%s" % (p[0], p[1][0] if len(p[1]) == 1 else "all")


@pytest.mark.parametrize("case", PARAMS, ids=_ids)
def test_model_equals_oracle_on_the_shared_blocks(oracle, case):
    size, names = case
    for name in names:
        d = invmodel.block(size, name)
        sp = invmodel.starting_points(size, name)
        bwt, lf, _ = oracle.oracle_bwt_block(d, sp)
        assert lf.size == (sp if size > 256 else 1)
        if name.startswith("eob_"):
            assert int(lf[0]) == int(name[4:]), (size, name)
        if name == "all_equal":
            assert int(lf[0]) == size
        m = invmodel.lf_model(bwt, lf)
        assert m.rc == 0 and m.one_cycle and m.powers_ok.all(), (size, name)
        assert m.out.tobytes() == d.tobytes(), (size, name)
        assert int(m.walk[size]) == int(lf[0]) and int(m.LF[int(lf[0])]) == 0
        rc, back = oracle.oracle_inverse_bwt_block(bwt, lf)
        assert rc == 0 and back.tobytes() == d.tobytes(), (size, name)


def test_model_equals_oracle_on_the_power_blocks(oracle):
    cases = [(size, n_lf, d) for size in invmodel.POWER_SIZES for n_lf, d in invmodel.power_blocks(size)]
    cases += [(size, n_lf, invmodel.plain_block(size, n_lf)) for size, n_lf in invmodel.OFF_BY_ONE]
    for size, n_lf, d in cases:
        bwt, lf, _ = oracle.oracle_bwt_block(d, n_lf)
        m = invmodel.lf_model(bwt, lf)
        assert lf.size == n_lf and m.rc == 0 and m.out.tobytes() == d.tobytes(), (size, n_lf)
        rc, back = oracle.oracle_inverse_bwt_block(bwt, lf)
        assert rc == 0 and back.tobytes() == d.tobytes(), (size, n_lf)


def test_block_with_eob_at_every_count_of_starting_points(oracle):
    rng = np.random.default_rng(5)
    for size in (1, 2, 63, 64, 65, 257, 513, 4097):
        for eob in invmodel.eobs(size):
            for sp in (1, 8, 256):
                d = invmodel.block_with_eob(size, eob, rng, sigma=int(rng.choice([2, 4, 256])))
                bwt, lf, _ = oracle.oracle_bwt_block(d, sp)
                assert int(lf[0]) == eob, (size, eob, sp)
                m = invmodel.lf_model(bwt, lf)
                assert m.rc == 0 and m.out.tobytes() == d.tobytes()


def test_model_on_the_reference_goldens():
    for c in json.load(open(os.path.join(G, "bwt_small.json")))["cases"]:
        data = base64.b64decode(c["input"])
        bwt = np.frombuffer(base64.b64decode(c["bwt"]), np.uint8)
        m = invmodel.lf_model(bwt, c["lf"])
        assert m.rc == 0 and m.out.tobytes() == data, c["name"]


def _same_verdict(oracle, bwt, lf):
    """The oracle's walk refuses (-3: a power off its place, -4: the walk is not one cycle) what the model refuses,
    and gives the model's bytes otherwise."""
    m = invmodel.lf_model(bwt, lf)
    rc, back = oracle.oracle_inverse_bwt_block(bwt, lf)
    if m.rc == 0:
        assert rc == 0 and back.tobytes() == m.out.tobytes()
    else:
        assert m.rc == -4 and rc in (-3, -4)
        assert (rc == -4) == (not m.one_cycle)
    return m


@pytest.mark.parametrize("size", invmodel.DAMAGE_SIZES)
def test_controlled_damage_is_what_it_says(oracle, size):
    d = invmodel.block(size, "random256") if size != 4096 else invmodel.block(size, "random2")
    for sp in (8, 1):
        bwt, lf, _ = oracle.oracle_bwt_block(d, sp)
        two = invmodel.damage_two_cycles(bwt, lf)
        m = _same_verdict(oracle, two, lf)
        assert m.rc == -4 and invmodel.cycles_without_splitter(m.LF)[0] == 2
        lone = invmodel.damage_cycle_without_splitter(bwt, lf)
        m = _same_verdict(oracle, lone, lf)
        assert m.rc == -4 and invmodel.cycles_without_splitter(m.LF) == (2, 1)
        one = invmodel.damage_one_cycle(bwt, lf)
        m = _same_verdict(oracle, one, lf)
        assert m.one_cycle and int((one != bwt).sum()) == 4
        assert (m.rc == 0) == (sp == 1 or bool(m.powers_ok.all()))
        if sp == 1:
            assert m.out.tobytes() != d.tobytes()
        for eob in (1, size, (int(lf[0]) + 777) % size + 1, int(lf[0]) + 1):
            if eob <= size:
                _same_verdict(oracle, bwt, [eob] + list(lf[1:]))


def test_powers_off_by_one_and_arguments(oracle):
    d = invmodel.block(510, "random256")
    bwt, lf, _ = oracle.oracle_bwt_block(d, 8)
    for k in range(1, 8):
        for delta in (-1, 1):
            bad = lf.copy()
            bad[k] = int(lf[k]) + delta
            if 0 <= int(lf[k]) + delta <= d.size:
                m = _same_verdict(oracle, bwt, bad)
                assert m.rc == -4 and m.one_cycle and not m.powers_ok[k - 1] and m.powers_ok.sum() == 6
    assert invmodel.lf_model(bwt, []).rc == -1 and invmodel.lf_model(bwt, [0] * 257).rc == -1
    assert invmodel.lf_model(bwt, [d.size + 1]).rc == -1
    assert invmodel.lf_model(bwt, [int(lf[0]), d.size + 1]).rc == -4
    # more powers than rows: x = 0, no power can be at index -1
    d5 = invmodel.block_with_eob(5, 3, np.random.default_rng(1))
    b5, l5, _ = oracle.oracle_bwt_block(d5, 1)
    assert invmodel.lf_model(b5, l5).rc == 0
    m = invmodel.lf_model(b5, [3] + [0] * 255)
    assert m.rc == -4 and m.one_cycle and not m.powers_ok.any()


def test_a_power_after_the_last_splitter_exists(oracle):
    """The case the GPU file uses for the wrap branch of the check (size 257, 256 powers, x = 1)."""
    d, bwt, lf, ks = invmodel.wrap_case(lambda data, sp: oracle.oracle_bwt_block(data, sp)[:2])
    m = invmodel.lf_model(bwt, lf)
    assert lf.size == 256 and int(lf[0]) % invmodel.SPLIT and m.rc == 0 and m.out.tobytes() == d.tobytes()
    last = max(int(m.pos[r]) for r in range(0, d.size + 1, invmodel.SPLIT))
    assert ks and all(int(m.pos[int(lf[k])]) == k - 1 > last for k in ks)
