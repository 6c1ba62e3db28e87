"""The Schnorr case set (tests/_schnorr_cases.py) against the host verifier, and the --sig-audit flag.  No GPU."""
import argparse

from _schnorr_cases import DRAWS, cases, challenge, host_status, point

from biscotti_amd.protocol.config import RunConfig, add_framework_flags, add_reference_flags, config_from_args


def test_expected_statuses_agree_with_the_host_verifier():
    cs = cases()
    keys, messages = cs["keys"], cs["messages"]
    assert len(cs["cases"]) >= 120
    seen = set()
    for case in cs["cases"]:
        got = host_status(case, keys, messages)
        if got is None:
            assert case.expect == 4, case.name
        else:
            assert got == case.expect, (case.name, got, case.expect)
        seen.add(case.expect)
    assert seen == {0, 1, 2, 4}


def test_the_edges_are_in_the_set():
    cs = cases()
    n = cs["order"]
    valid = [c for c in cs["cases"] if c.expect == 0]
    r_top = [c for c in valid if c.sig[32] > 0x80]
    c_top = [c for c in valid if c.sig[0] > 0x80]
    assert len(r_top) >= 5 and len(c_top) >= 5          # the carry into window 32
    rs = {int.from_bytes(c.sig[32:], "big") for c in valid}
    for r in (1, n - 1, int.from_bytes(b"\x80" * 32, "big"), int.from_bytes(b"\x81" * 32, "big"), 2 ** 8 - 1,
              2 ** 64 - 1, 2 ** 255 - 1):
        assert r in rs
    assert bytes(64) in cs["keys"]                       # the point at infinity as a key
    # a forged pair whose T is the point at infinity
    assert any(point(r, c, cs["keys"][k]) == bytes(64) for r, c, k in cs["scalars"])


def test_no_case_needs_more_than_the_draw_cap():
    cs = cases()
    keys, messages, n = cs["keys"], cs["messages"], cs["order"]
    most = 0
    for case in cs["cases"]:
        c, r = int.from_bytes(case.sig[:32], "big"), int.from_bytes(case.sig[32:], "big")
        if c >= n or r >= n or not (0 <= case.key_idx < len(keys) and 0 <= case.msg_idx < len(messages)):
            continue
        _, draws = challenge(point(r, c, keys[case.key_idx]), messages[case.msg_idx])
        most = max(most, draws)
    assert 1 <= most <= DRAWS


def test_sig_audit_flag():
    RunConfig(sig_audit=True).validate()
    ap = argparse.ArgumentParser()
    add_reference_flags(ap)
    add_framework_flags(ap)
    assert not config_from_args(ap.parse_args([])).sig_audit and not RunConfig().sig_audit
    assert config_from_args(ap.parse_args(["--sig-audit"])).sig_audit
