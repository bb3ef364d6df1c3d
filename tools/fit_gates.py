#!/usr/bin/env python
"""Prints what tests/test_gpu_fit.py records as E32: the error of the fit's oracle (tests/_fit_oracle.py) run in fp32 on
the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.  The GPU gates are 4 x these.  Needs no
GPU; also prints the oracle's recovery figures (start, after 10 and after 20 iterations) for DESIGN.md 12."""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_oracle as FO
    import _fit_cases as G

    T_ = G.T_
    cases = [((B, V), G.host_model(V), G.case(B, V)) for V in (37, 778) for B in (1, 3, 65)]
    cases.append((("edge",), G.host_model("edge"), G.edge_batch()))
    for key, m, (P, x, jac) in cases:
        x32, j32 = FO.joints_jac(m, T_(P))
        print(f'("x", {", ".join(map(repr, key))}): {FO.rel(x32.numpy(), x):.3e}, '
              f'("jac", {", ".join(map(repr, key))}): {FO.rel(j32.numpy(), jac):.3e},')
    ones = torch.ones(6, 21)
    for V in (37, 778):
        m = G.host_model(V)
        T, P1, Ps, c = G.step_case(V)
        P32, _, acc = FO.lm(m, T, ones, G.JOINT_MAP, P1.float(), 1, lambda0=1e-2)
        print(f'("step", {V}): {FO.rel(P32.numpy(), Ps.numpy()):.3e},   # accepted {acc.tolist()}')
    # the cost: the oracle's cost function in fp32 against fp64 at the oracle's own iterate after k iterations (V = 778)
    m = G.host_model(778)
    P, T, P0, Pf, want, hist = G.recovery_case(778)
    for k in (1, 2, 5, 10):
        Pk = FO.lm(m, T.double(), ones.double(), G.JOINT_MAP, P0, k)[0].float()
        with torch.no_grad():
            c32 = FO.cost(m, Pk, T, ones, G.JOINT_MAP, 1e-6, 1e-6)
            c64 = FO.cost(m, Pk.double(), T.double(), ones.double(), G.JOINT_MAP, 1e-6, 1e-6)
        print(f'("cost", {k}): {FO.rel(c32.numpy(), c64.numpy()):.3e},')
    for V in (37, 778):
        m = G.host_model(V)
        P, T, P0, Pf, want, hist = G.recovery_case(V)
        P10 = FO.lm(m, T.double(), ones.double(), G.JOINT_MAP, P0, 10)[0]
        P32 = FO.lm(m, T, ones, G.JOINT_MAP, P0.float(), 20)[0]
        mm = lambda q: (1e3 * FO.rms(m, q, T, G.JOINT_MAP)).numpy().round(4).tolist()
        print(f"recovery V {V}: joint RMS in mm, start {mm(P0)}, fp64 oracle after 10 {mm(P10)}, after 20 {mm(Pf)}, "
              f"the oracle in fp32 after 20 {mm(P32)}")


if __name__ == "__main__":
    main()
