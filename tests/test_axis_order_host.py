"""K1's banded workgroup order (axis_block_order, csrc/aai_plan.hpp) on the host: a few lines of C++ compiled against the header the
kernel includes print the map for every grid of gridX 1..20 x gridY 1..80, and the three properties the kernel relies on are checked:
the map is a bijection of [0, gridX gridY) onto the grid (no row block dropped or served twice, nothing out of range); in the banded
part all gridX strip blocks of a row block come from workgroups with one value of b % 8, and eight consecutive row blocks take the
eight values; the row blocks past the last whole group of eight keep launch order."""
import os
import subprocess

import numpy as np
import pytest

from conftest import BUILD, ROOT

PROBE = r"""
#include <cstdio>
#include "aai_plan.hpp"
int main()
{
    for (unsigned gx = 1; gx <= 20; ++gx)
        for (unsigned gy = 1; gy <= 80; ++gy)
            for (unsigned b = 0; b < gx * gy; ++b) {
                int bx = -1, by = -1;
                aai::axis_block_order(b, gx, gy, &bx, &by);
                printf("%u %u %u %d %d\n", gx, gy, b, bx, by);
            }
    return 0;
}
"""


@pytest.fixture(scope="module")
def order_table():
    os.makedirs(BUILD, exist_ok=True)
    src, exe = os.path.join(BUILD, "axis_order_probe.cpp"), os.path.join(BUILD, "axis_order_probe")
    with open(src, "w") as f:
        f.write(PROBE)
    csrc = os.path.join(ROOT, "area_average_interpolation_amd", "csrc")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    t = np.array(out.split(), dtype=np.int64).reshape(-1, 5)
    assert t.shape[0] == sum(gx * gy for gx in range(1, 21) for gy in range(1, 81))
    return t


def grids(t):
    """(gridX, gridY, bx[b], by[b]) of every grid of the table, b ascending"""
    key = t[:, 0] * 1000 + t[:, 1]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], t.shape[0]]):
        gx, gy = int(t[s, 0]), int(t[s, 1])
        assert e - s == gx * gy and np.array_equal(t[s:e, 2], np.arange(gx * gy))
        yield gx, gy, t[s:e, 3], t[s:e, 4]


def test_order_is_a_bijection(order_table):
    n = 0
    for gx, gy, bx, by in grids(order_table):
        assert bx.min() >= 0 and bx.max() < gx and by.min() >= 0 and by.max() < gy, (gx, gy)
        assert np.array_equal(np.sort(by * gx + bx), np.arange(gx * gy)), (gx, gy)
        n += 1
    assert n == 20 * 80


def test_banded_part_gives_each_label_whole_row_blocks(order_table):
    for gx, gy, bx, by in grids(order_table):
        banded = gy // 8 * 8
        b = np.arange(gx * gy)
        label = b % 8
        head = b < banded * gx
        # the banded part serves exactly the first `banded` row blocks
        assert np.array_equal(np.unique(by[head]), np.arange(banded)), (gx, gy)
        for row in range(banded):
            of_row = head & (by == row)
            assert of_row.sum() == gx and np.unique(label[of_row]).size == 1, (gx, gy, row)
            assert label[of_row][0] == row % 8, (gx, gy, row)                 # eight consecutive row blocks take the eight values
            # ... from ONE group of 8 gridX consecutive workgroups, strip block by strip block
            assert np.array_equal(b[of_row] // (8 * gx), np.full(gx, row // 8)) and np.array_equal(bx[of_row], np.arange(gx)), (gx, gy, row)


def test_remainder_keeps_launch_order(order_table):
    for gx, gy, bx, by in grids(order_table):
        b = np.arange(gx * gy)
        tail = b >= gy // 8 * 8 * gx
        assert np.array_equal(bx[tail], b[tail] % gx) and np.array_equal(by[tail], b[tail] // gx), (gx, gy)
        if gy < 8:
            assert tail.all()
