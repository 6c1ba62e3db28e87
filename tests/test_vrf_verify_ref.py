"""The plain-Python ECVRF verifier (_ecvrf_verify_ref.py) pinned to RFC 9381 and to the host runtime's
vrf_verify on the tamper set that tests/test_gpu_vrf_verify.py runs on the device.

The counts asserted below are properties of the reference on that set: a verifier that rejects nothing, or
everything, cannot agree with it."""
from collections import Counter

import _ecvrf_ref as E
import _ecvrf_verify_ref as VR
import test_vrf_edges as V
from biscotti_amd.native import rt


def test_reference_verifies_the_rfc9381_vector():
    _, pk, alpha, pi = VR.rfc_case()
    assert alpha == b""
    assert VR.verify(pk, alpha, pi) == (0, bytes.fromhex(V.RFC_BETA))
    assert rt().vrf_verify(pk, alpha, pi) == bytes.fromhex(V.RFC_BETA)
    assert VR.verify(pk, alpha, pi, expect=bytes.fromhex(V.RFC_BETA))[0] == 0
    assert VR.verify(pk, alpha, pi, expect=bytes(64)) == (5, bytes.fromhex(V.RFC_BETA))


def test_reference_equals_host_on_the_tamper_set():
    R = rt()
    for (name, pk, alpha, pi), (status, beta) in zip(VR.cases(), VR.reference()):
        host = R.vrf_verify(pk, alpha, pi)
        if host is None:
            assert status in (1, 2, 3, 4) and beta == VR.ZERO_BETA, name
        else:
            assert status == 0 and beta == host, name


def test_tamper_set_statuses():
    cases, ref = VR.cases(), VR.reference()
    by = {name: st for (name, *_), (st, _) in zip(cases, ref)}
    flips = [st for st, _ in ref[:VR.N_FLIPS]]
    assert Counter(flips) == {4: 507, 2: 129, 3: 4}
    assert all(i < 256 for i, st in enumerate(flips) if st == 2)   # Gamma's bits
    assert all(i >= 384 for i, st in enumerate(flips) if st == 3)   # s's bits
    assert by["s+L"] == 3 and by["wrong-message"] == 4 and by["wrong-key"] == 4
    assert by["pk-P+1"] == 1 and by["gamma-P+1"] == 2 and by["untampered"] == 0
    for nm in ("0", "L", "L-1", "8"):
        for j in range(len(V.CRAFTED_ALPHAS)):
            assert by[f"crafted-{nm}-{j}"] == 0, nm
    # the identity as Gamma and as the public key: the formula accepts it
    x0 = [c for c in cases if c[0] == "crafted-0-0"][0]
    assert x0[1] == E.enc(E.IDENTITY) and x0[3][:32] == E.enc(E.IDENTITY)
    assert len(cases) == VR.N_FLIPS + 6 + 2 * len(V.CRAFTED_X)
