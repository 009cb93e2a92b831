"""The two-wave kernel's request phase and register forms of the front end (dwbc_cycle2p.h, dwbc_front.h) through the host build of
the same source (tests/emu, both roles in turn), against the oracle at the bar tests/test_launch_flavours.py uses for this kernel:
one, two and three declared contacts, every flag pattern of each on every state of tests/pair_prologue_cases.py -- three flags on
this two-contact kernel included (status 0, zero outputs)."""
import numpy as np
import pytest

from tests import cases
from tests import pair_prologue_cases as pc
from tests.emu.emu import Emu


@pytest.mark.parametrize("n", pc.DECLARED)
def test_oracle_solves_every_compared_case(n):
    """the reference alone: status 1 and torques that differ between the flag patterns, so a flag read from a neighbour shows"""
    ref, pat = pc.reference(n), pc.patterns(n)
    few = pat.sum(axis=1) <= pc.MAX_ACTIVE
    assert (ref["status"][few] == 1).all(), ref["status"]
    tau = ref["tau"][few].sum(axis=2)  # (patterns, states, m)
    for a in range(len(tau)):
        for b in range(a + 1, len(tau)):
            assert np.abs(tau[a] - tau[b]).max(axis=1).min() > 1e-3, (pat[few][a], pat[few][b])


@pytest.mark.parametrize("n", pc.DECLARED)
def test_emulated_two_wave_cycle_every_flag_pattern(n):
    q, fstar = pc.states()
    pat = pc.patterns(n)
    P = len(pat)
    pi, si = np.repeat(np.arange(P), pc.NSTATES), np.tile(np.arange(pc.NSTATES), P)
    r = Emu(cases.URDF, cases.CONTACTS_4[:n], cases.TASKS_2LEVEL, cases.TAU_LIM).run(q[si], pat[pi], fstar[si], compact="pair")
    pc.check(f"emu[{n} declared]", n, pi, si, r["tau"], r["wrench"], r["status"])
