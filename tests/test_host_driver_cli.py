"""The C++ host driver's command line where no GPU is needed: usage errors,
unknown options and parameter sets, and the usage text's option list."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ntt-gpu-qtesla_amd", "bin", "ntt_main")
USAGE_RC = 255   # the driver returns -1
BANNER = "NTT Parameters==> NTTSIZE: 1024 P: 8404993 psi: 2083362 batch: 2\n"


@pytest.fixture(scope="module")
def run():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()

    def run(*args):
        return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    return run


@pytest.fixture(scope="module")
def usage(run):
    r = run()
    assert r.returncode == USAGE_RC
    assert r.stdout.startswith("usage: ntt_main -speedgpu {") and r.stdout.count("\n") == 1, r.stdout
    return r.stdout


def test_usage_lists_every_option(usage):
    (options,) = re.findall(r"-speedgpu \{([0-9,]+)\}", usage)
    assert sorted(int(x) for x in options.split(",")) == [4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    for flag in ("-param ref|p-I|p-III|p-III-4096|p-III-8192", "-batch B", "-reps R", "-k K", "-d D", "-leg a|b", "-r seed",
                 "-pcie", "-debug"):
        assert f"[{flag}]" in usage, usage


@pytest.mark.parametrize("args", [
    ("-speedgpu", "6", "-batch"),          # a flag with its value missing
    ("-speedgpu", "6", "-param"),
    ("-speedgpu", "6", "-bogus"),          # an unknown flag
    ("-speedgpu", "6", "-param", "ref", "extra"),
], ids=" ".join)
def test_usage_errors(run, usage, args):
    r = run(*args)
    assert r.returncode == USAGE_RC
    assert r.stdout == usage, r.stdout


def test_unknown_option_prints_banner_then_usage(run, usage):
    r = run("-speedgpu", "99", "-param", "ref")
    assert r.returncode == USAGE_RC
    assert r.stdout == BANNER + usage, r.stdout


def test_unknown_parameter_set(run):
    r = run("-speedgpu", "6", "-param", "nope")
    assert r.returncode == USAGE_RC
    assert "unknown parameter set" in r.stderr and r.stdout == "", r.stdout + r.stderr
