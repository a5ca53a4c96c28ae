"""The C++ host driver (ntt-gpu-qtesla_amd/host/ntt_main.cpp, the only C++
caller of the C ABI) on the GPU: every option's own check reports Identical.

Each case is one short child process, run after the previous one.
"""
import json
import os
import re
import subprocess

import pytest

from conftest import LARGE_SETS, PARAM_SETS

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntt-gpu-qtesla_amd", "bin", "ntt_main")


def _run(opt, ps, batch, *extra):
    return subprocess.run([EXE, "-speedgpu", str(opt), "-param", ps, "-batch", str(batch), *extra], capture_output=True,
                          text=True, timeout=120)


def _identical(r):
    """return code 0, at least one result line, every one of them `Identical.`; returns the result lines"""
    assert r.returncode == 0, r.stdout + r.stderr
    verdicts = [l for l in r.stdout.splitlines() if l.endswith(("Identical.", "Incorrect result."))]
    assert verdicts and all(l.endswith("Identical.") for l in verdicts), r.stdout
    assert "Incorrect result." not in r.stdout, r.stdout
    return verdicts


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_host_driver_kat(ps):
    """The C++ host driver (reference CLI) reports the all-ones KAT as Identical."""
    for opt in ("6", "7"):
        r = _run(opt, ps, "4")
        assert r.returncode == 0, r.stderr
        assert "Identical." in r.stdout, r.stdout
    r = _run("9", ps, "1000", "-r", "5")
    assert r.returncode == 0 and "Identical." in r.stdout, r.stdout + r.stderr
    for opt, batch in (("10", "5000"), ("11", "7")):   # host pipeline (2 chunks at n=1024), Nussbaumer mod 2^32-1
        r = _run(opt, ps, batch)
        assert r.returncode == 0 and "Identical." in r.stdout, r.stdout + r.stderr
    # per-call latency option: one JSON line per entry point, small batch
    r = _run("12", ps, "1", "-reps", "50")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [d["op"] for d in lines] == ["poly_ntt", "poly_invntt", "poly_mul"]
    assert all(0 < d["back_to_back_us"] < 1e4 and d["calls"] == 50 for d in lines)


@pytest.mark.parametrize("ps", LARGE_SETS)
def test_large_host_driver_kat(ps):
    """The C++ host driver (reference CLI) at n = 4096 / 8192: CT-GS
    composition and fused product report the all-ones KAT as Identical, the
    transform round trip and the host pipeline pass; Nussbaumer (option 11)
    fails with the library's NTT_ERR_PARAM."""
    for opt, batch in (("6", "4"), ("7", "4"), ("9", "300"), ("10", "1500")):
        r = _run(opt, ps, batch, *(["-r", "5"] if opt == "9" else []))
        assert r.returncode == 0 and "Identical." in r.stdout, r.stdout + r.stderr
    r = _run("11", ps, "2")
    assert r.returncode != 0


# options 13 / 14.  Batch 1: head and tail are the same polynomial; 3: odd, the
# n = 1024 half-wave tail; 300: above 256, so the tail window starts at
# batch - 256 and differs from the head.
@pytest.mark.parametrize("operands", ["ones", "random"])
@pytest.mark.parametrize("batch", [1, 3, 300])
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("opt", [13, 14])
def test_fused_products(opt, ps, batch, operands):
    """poly_mul_ntt_k / poly_mul_ntt_kl against what they replace: all-ones
    operands take the KAT branch, -r 7 the fused == baseline branch."""
    r = _run(opt, ps, batch, "-reps", "1", *(["-r", "7"] if operands == "random" else []))
    (verdict,) = _identical(r)
    assert verdict.startswith("fused ==" if operands == "random" else "all-ones KAT"), r.stdout
    k = {"ref": 1, "p-I": 4, "p-III": 5}[ps]
    assert f"Batch Size is {batch}, k = {k}" in r.stdout, r.stdout


@pytest.mark.parametrize("opt", [13, 14])
def test_fused_products_k_override(opt):
    r = _run(opt, "p-III", 3, "-reps", "1", "-r", "7", "-k", "2")
    _identical(r)
    assert "Batch Size is 3, k = 2" in r.stdout, r.stdout


ROUND_A = "poly_round GPU."
ROUND_B = "poly_mul_ntt_kl_round GPU."
ROUND_A_LINES = ("poly_round hi+norms :", "poly_round hi       :", "poly_round norms    :", "poly_pointwise      :")


def _leg_a_lines(out):
    return [l for l in out.splitlines() if l.startswith(ROUND_A_LINES)]


@pytest.mark.parametrize("batch", [3, 300])
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_round_both_legs(ps, batch):
    """option 15: leg (a) prints its four timing lines, leg (b) compares the
    fused product with poly_mul_ntt_kl + poly_round."""
    r = _run(15, ps, batch, "-reps", "1", "-r", "7")
    (verdict,) = _identical(r)
    assert verdict.startswith("fused == poly_mul_ntt_kl + poly_round"), r.stdout
    assert ROUND_A in r.stdout and ROUND_B in r.stdout, r.stdout
    assert [l[:21] for l in _leg_a_lines(r.stdout)] == list(ROUND_A_LINES), r.stdout


def test_round_single_leg():
    r = _run(15, "p-I", 3, "-reps", "1", "-r", "7", "-leg", "a")
    assert r.returncode == 0, r.stdout + r.stderr
    assert ROUND_B not in r.stdout and len(_leg_a_lines(r.stdout)) == 4, r.stdout
    r = _run(15, "p-I", 3, "-reps", "1", "-r", "7", "-leg", "b")
    _identical(r)
    assert ROUND_A not in r.stdout and ROUND_B in r.stdout, r.stdout


def test_round_large_set_runs_leg_a_only():
    r = _run(15, LARGE_SETS[0], 3, "-reps", "1", "-r", "7")
    assert r.returncode == 0, r.stdout + r.stderr
    assert ROUND_B not in r.stdout and len(_leg_a_lines(r.stdout)) == 4, r.stdout


@pytest.mark.parametrize("ps", ["p-I", "p-III"])
def test_xof_and_challenge(ps):
    """option 16: both legs' banners, and a digest that depends on the seed alone."""
    digests = []
    for _ in range(2):
        r = _run(16, ps, 3, "-reps", "1", "-r", "1")
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ntt_xof GPU." in r.stdout and "poly_challenge GPU." in r.stdout, r.stdout
        (m,) = re.findall(r"^out\[0\] +: ([0-9a-f]+)$", r.stdout, re.M)
        assert len(m) == 64, r.stdout
        digests.append(m)
    assert digests[0] == digests[1]


def test_xof_rejects_large_set():
    r = _run(16, LARGE_SETS[0], 3, "-reps", "1", "-r", "1")
    assert r.returncode != 0
    assert "-speedgpu 16" in r.stderr and "n = 1024 / 2048" in r.stderr, r.stderr


def test_composed_and_speed_suite():
    """option 4 (CT-CT) and option 8 (5 x CT-GS, then 5 x fused), all-ones KAT"""
    assert len(_identical(_run(4, "ref", 4, "-reps", "1"))) == 1
    r = _run(8, "ref", 4, "-reps", "1")
    assert len(_identical(r)) == 10
    assert r.stdout.count("test_NTT_negacyclic CT-GS GPU.") == 5 and r.stdout.count("test_NTT_negacyclic fused GPU.") == 5
