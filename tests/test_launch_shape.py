"""The library's one launch-shape rule (ntt-gpu-qtesla_amd/csrc/launch_shape.hpp),
without a GPU: a stand-alone host program that includes only that header is
compiled and fed (items, per, cus, per_cu, max) tuples; its (grid, chunk)
must equal the rule restated here, cover all the work, leave no workgroup
empty and fit a 32-bit grid.  The capped-grid rule likewise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ntt-gpu-qtesla_amd", "csrc", "launch_shape.hpp")

MAIN = r"""
#include "launch_shape.hpp"

#include <cstdio>

// the rule is usable in constant expressions
static_assert(qntt::launch_shape(1, 8, 256, 4, 16).grid == 1 && qntt::launch_shape(1, 8, 256, 4, 16).chunk == 1, "");
static_assert(qntt::capped_grid(257, 256, 256, 8) == 2, "");

int main()
{
    char kind;
    unsigned long long a, b, c, d, e;
    while (std::scanf(" %c %llu %llu %llu %llu %llu", &kind, &a, &b, &c, &d, &e) == 6) {
        if (kind == 's') {
            const qntt::LaunchShape l = qntt::launch_shape(a, b, c, d, e);
            std::printf("%u %u\n", l.grid, l.chunk);
        } else {
            std::printf("%u 0\n", qntt::capped_grid(a, b, c, d));
        }
    }
    return 0;
}
"""

# (per workgroup and pass, workgroups per CU, max chunk) of every launch site
SITES = {
    "batch transforms, n <= 2048": (8, 4, 16),
    "poly_mul, 512-thread workgroup": (8, 4, 16),
    "poly_mul, 1024-thread workgroup": (16, 4, 16),
    "poly_mul_ntt_k": (6, 4, 4),
    "poly_mul_ntt_kl / _kl_round": (4, 4, 4),
    "n = 4096 transforms": (16, 2, 16),
    "n = 8192 transforms": (8, 2, 16),
    "n = 4096 products": (4, 2, 16),
    "n = 4096 products, NTT-domain operand": (8, 2, 16),
    "n = 8192 products, 2 slots": (2, 2, 16),
    "n = 8192 products, 4 slots": (4, 2, 16),
    "poly_round": (1, 8, 4),
    "Nussbaumer mod q": (1, 2, 1),
    "Nussbaumer mod 2^32 - 1, n = 2048": (1, 2, 16),
}
CUS = (1, 256, 304)
# (wg, cap): poly_pointwise, ntt_fill_uniform, the n = 4096 / 8192 bit-reversal copy
CAPPED = ((256, 8), (256, 16), (1, 64))


def shape_tuples():
    out = []
    for per, per_cu, mx in SITES.values():
        for cus in CUS:
            T = per * cus * per_cu
            for items in (1, T - 1, T, T + 1, 2 * T, T * mx - 1, T * mx, T * mx + 1, 2 ** 31 - 1):
                if items >= 1:
                    out.append((items, per, cus, per_cu, mx))
    return sorted(set(out))


def capped_tuples():
    out = []
    for wg, cap in CAPPED:
        for cus in CUS:
            for count in (1, wg, wg + 1, wg * cus * cap, wg * cus * cap + 1):
                out.append((count, wg, cus, cap))
    return sorted(set(out))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("launch_shape")
    src, exe = d / "main.cpp", d / "launch_shape"
    src.write_text(MAIN)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    shapes, capped = shape_tuples(), capped_tuples()
    text = "".join("s %d %d %d %d %d\n" % t for t in shapes) + "".join("c %d %d %d %d 0\n" % t for t in capped)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(shapes) + len(capped)
    return dict(zip(shapes, rows[:len(shapes)])), dict(zip(capped, (g for g, _ in rows[len(shapes):])))


def test_header_is_free_of_hip():
    includes = re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', open(HEADER).read())
    assert sorted(includes) == ["cstddef", "cstdint"]


def test_launch_shape_rule(answers):
    shapes, _ = answers
    assert len(shapes) >= 200   # 14 sites x 3 device sizes x 9 item counts, less the duplicates
    for (items, per, cus, per_cu, mx), (grid, chunk) in shapes.items():
        # the rule, restated
        want_chunk = min(max(items // (per * cus * per_cu), 1), mx)
        want_grid = -(-items // (per * want_chunk))
        where = f"items={items} per={per} cus={cus} per_cu={per_cu} max={mx}"
        assert (grid, chunk) == (want_grid, want_chunk), where
        assert 1 <= chunk <= mx, where
        assert grid * per * chunk >= items, f"{where}: work left over"
        assert (grid - 1) * per * chunk < items, f"{where}: an empty workgroup"
        assert grid < 2 ** 32, where


def test_chunk_grows_only_with_enough_workgroups(answers):
    """Below max chunk, a chunk of c > 1 leaves at least per_cu workgroups per CU."""
    shapes, _ = answers
    for (items, per, cus, per_cu, mx), (grid, chunk) in shapes.items():
        if chunk > 1:
            assert grid >= cus * per_cu, (items, per, cus, per_cu, mx)


def test_capped_grid_rule(answers):
    _, capped = answers
    for (count, wg, cus, cap), grid in capped.items():
        assert grid == min(-(-count // wg), cus * cap), (count, wg, cus, cap)
        assert 1 <= grid <= cus * cap
