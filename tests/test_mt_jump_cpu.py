"""Jump polynomials of MT19937 on the host (csrc/mt19937_jump.h through hp_mt_jump_poly): no device needed -- the library
loads anywhere, only hp_ctx_create wants a GPU.  Everything is compared with numpy's legacy RandomState, never with the
library's own generator."""
import ctypes as C
import re

import numpy as np
import pytest

from rl_arm_under_sparse_reward_amd import _lib

DEG = 19937
JUMPS = (1, 623, 624, 625, 19937, 624 * 1000, 10 ** 7 + 3)
SEEDS = (0, 125, 2 ** 32 - 1)


def jump_poly(n):
    limbs = np.zeros(312, np.uint64)
    assert _lib.load().hp_mt_jump_poly(C.c_uint64(n), limbs.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, _lib.last_error()
    return limbs


def coefficients(limbs):
    """exponents of the set coefficients, ascending"""
    return np.flatnonzero(np.unpackbits(limbs.view(np.uint8), bitorder="little"))


def temper(y):
    y = y.astype(np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def raw_blocks(rs, n_blocks):
    """The next `n_blocks` key blocks of `rs` as raw (untempered) words, read off get_state() block by block: z_0 is the first
    word of the block AFTER the one rs holds (a seeded key is not generated: the recurrence never reads 31 bits of key[0])."""
    assert rs.get_state()[2] == 624
    out = np.empty((n_blocks, 624), np.uint32)
    for b in range(n_blocks):
        rs.bytes(4)                        # twists: the key is now the next block, word 0 consumed
        out[b] = rs.get_state()[1]
        rs.bytes(4 * 623)                  # to the end of that block
    return out.reshape(-1)


def words_after(seed, skip, count):
    """tempered words skip .. skip + count of the generated stream of `seed`, from numpy"""
    rs = np.random.RandomState(seed)
    assert rs.get_state()[2] == 624
    rs.bytes(4 * skip)
    return np.frombuffer(rs.bytes(4 * count), dtype="<u4")


@pytest.mark.parametrize("n", JUMPS)
def test_jump_polynomial_reproduces_the_block_n_words_ahead(n):
    """z_{n + k} = XOR over the set coefficients c_i of x^n mod phi of z_{k + i}, k < 624: the XOR of shifted windows of the 33
    blocks behind a key is the key block n words further on, as RandomState reaches it by drawing n words."""
    exps = coefficients(jump_poly(n))
    assert exps.size and exps[-1] < DEG
    for seed in SEEDS:
        z = raw_blocks(np.random.RandomState(seed), 33)
        assert z.size >= DEG + 623
        block = np.zeros(624, np.uint32)
        for i in exps:
            block ^= z[i:i + 624]
        assert np.array_equal(temper(block), words_after(seed, n, 624)), (n, seed)


def test_small_jumps_are_monomials_and_the_polynomials_compose():
    for n in (0, 1, 623, 19936):
        assert list(coefficients(jump_poly(n))) == [n]
    assert coefficients(jump_poly(DEG)).size > 1       # x^19937 is the first power that phi folds


def test_phi_has_degree_19937_and_annihilates_an_independent_sequence():
    """phi = x^19937 + (x^19937 mod phi).  The library derives it from seed 5489's output; seeds 1 and 4357 were not used."""
    low = coefficients(jump_poly(DEG))
    assert low[-1] < DEG and low[0] == 0               # constant term 1: the transition is invertible
    phi = np.concatenate([low, [DEG]])
    assert phi.size == 135                             # the weight Matsumoto and Nishimura give for MT19937
    for seed in (1, 4357):
        z = raw_blocks(np.random.RandomState(seed), 34)
        acc = np.zeros(1024, np.uint32)
        for e in phi:
            acc ^= z[e:e + 1024]
        assert not acc.any(), seed
    # and it is the minimal one for this stream: a proper divisor cannot exist (phi is irreducible), spot-check that dropping
    # the top term does not annihilate
    acc = np.zeros(64, np.uint32)
    for e in low:
        acc ^= z[e:e + 64]
    assert acc.any()


def test_parallel_draw_threshold_is_the_headers():
    from conftest import REPO
    import os
    txt = open(os.path.join(REPO, "include", "rlarm_hip.h")).read()
    assert int(re.search(r"#define\s+HP_PARALLEL_DRAW_MIN_BATCH\s+(\d+)", txt).group(1)) == _lib.PARALLEL_DRAW_MIN_BATCH
