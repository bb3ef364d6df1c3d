#!/usr/bin/env python
"""Prints what tests/test_gpu_fit_verts.py records as E32: the error of the vertex fit's oracle (tests/_fit_verts_oracle.py)
run in fp32 on the CPU against its own fp64 run on the test's inputs, max |a - b| / max |b|.  The GPU gates are 4 x these.
Needs no GPU; also prints the oracle's recovery figures (start, after 20 iterations, and what a joints fit of the same
hands leaves on the vertices) for DESIGN.md."""
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _fit_oracle as FO
    import _fit_verts_oracle as VO
    import _fit_verts_cases as G

    T_ = G.T_
    cases = [((B, V), G.host_model(V), G.case(B, V)) for V in G.JAC_V for B in G.JAC_B]
    cases.append((("edge",), G.host_model("edge"), G.edge_case()))
    for key, m, (P, x, jac) in cases:
        x32, j32 = VO.verts_jac(m, T_(P))
        print(f'("verts", {", ".join(map(repr, key))}): {VO.rel(x32.numpy(), x):.3e}, '
              f'("jac", {", ".join(map(repr, key))}): {VO.rel(j32.numpy(), jac):.3e},')
    # the joints' Jacobian (tests/_fit_oracle.py) on the same inputs: the other side of the tips cross-check
    for V in G.FIT_V:
        P = G.case(3, V)[0]
        j64, j32 = FO.joints_jac(G.host_model(V), T_(P).double())[1], FO.joints_jac(G.host_model(V), T_(P))[1]
        print(f'("jjac", 3, {V}): {VO.rel(j32.numpy(), j64.numpy()):.3e},')
    P, Tv, P0, Pf, want, hist = G.layer_case()
    print(f"layer case: fp64 oracle after 20 {(1e3 * want).round(4).tolist()} mm")
    for V in G.FIT_V:
        m, ones = G.host_model(V), torch.ones(G.NB, V)
        Tv, P1, Ps, c = G.step_case(V)
        P32, _, acc = VO.lm(m, Tv, ones, P1.float(), 1, lambda0=1e-2)
        print(f'("step", {V}): {VO.rel(P32.numpy(), Ps.numpy()):.3e},   # accepted {acc.tolist()}')
    # the cost: the oracle's cost function in fp32 against fp64 at the oracle's own iterate after k iterations
    for V in G.FIT_V:
        m, ones = G.host_model(V), torch.ones(G.NB, V)
        P, Tv, P0, Pf, want, hist = G.recovery_case(V)
        for k in G.ITERS:
            Pk = VO.lm(m, Tv.double(), ones.double(), P0, k)[0].float()
            with torch.no_grad():
                c32 = VO.cost(m, Pk, Tv, ones, 1e-6, 1e-6)
                c64 = VO.cost(m, Pk.double(), Tv.double(), ones.double(), 1e-6, 1e-6)
            print(f'("cost", {V}, {k}): {VO.rel(c32.numpy(), c64.numpy()):.3e},')
    for V in G.FIT_V:
        m = G.host_model(V)
        P, Tv, P0, Pf, want, hist = G.recovery_case(V)
        _, _, left = G.joints_case(V)
        mm = lambda q: (1e3 * VO.rms(m, q, Tv)).numpy().round(4).tolist()
        print(f"recovery V {V}: vertex RMS in mm, start {mm(P0)}, fp64 oracle after 20 {mm(Pf)}; the joints oracle after 20 "
              f"leaves {(1e3 * left).round(4).tolist()}")


if __name__ == "__main__":
    main()
