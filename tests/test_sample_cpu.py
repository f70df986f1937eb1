"""The random numbers and the witness of gpcc_sample_batch on the CPU: the numpy Philox4x64-10 mirror (gpcc_amd.rng) against
Random123's known answer and numpy's Philox, csrc/gpcc_rng.h compiled for the host against the mirror (words, normals, row choices with
edge weights), and the parity bar of tests/_sample_witness.py against five injected slips."""
import os
import subprocess

import numpy as np
import pytest

import _sample_witness as SW
from gpcc_amd import rng, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpcc.jl_amd", "csrc")


def test_philox_known_answer():
    """Random123's kat_vectors: philox4x64-10, counter 0, key 0."""
    x = rng.philox4x64([0, 0, 0, 0], [0, 0])
    assert [int(v) for v in x] == [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]


@pytest.mark.parametrize("c,k", [([0, 0, 0, 0], [0, 0]), ([5, 7, 9, 11], [123, 456]), ([2**64 - 2, 3, 2**64 - 1, 1], [2**63 + 5, 0]),
                                 ([17, 0, 2**64 - 1, 1], [987654321, 0])])
def test_philox_against_numpy(c, k):
    """numpy's Philox increments the counter before each block: random_raw(4) of counter c is the block of c + 1."""
    bg = np.random.Philox(counter=np.array(c, dtype=np.uint64), key=np.array(k, dtype=np.uint64))
    ref = bg.random_raw(4)
    v = (c[0] + (c[1] << 64) + (c[2] << 128) + (c[3] << 192) + 1) % (1 << 256)
    c1 = [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]
    assert np.array_equal(rng.philox4x64(c1, k), ref.astype(np.uint64))


def test_normals_are_standard():
    z = rng.normals(7, 4000, np.arange(5), 3).ravel()
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    # the block of test index j is j // 4: prefixes in T agree, and the mixture row word gives other numbers
    assert np.array_equal(rng.normals(7, 9, [2], 3)[0], rng.normals(7, 4000, [2], 3)[0, :9])
    assert not np.array_equal(rng.normals(7, 8, [2], 3), rng.normals(7, 8, [2], rng.MIXROW))


_CPP = r'''
#include "gpcc_rng.h"
#include <cstdio>
#include <vector>
int main()
{
    const unsigned long long ctr[][4] = {{0, 0, 0, 0}, {5, 7, 9, 11}, {3, 2, ~0ULL, 1}, {~0ULL, ~0ULL, ~0ULL, ~0ULL}};
    const unsigned long long key[][2] = {{0, 0}, {123, 456}, {42, 0}, {~0ULL, 1}};
    for (int i = 0; i < 4; ++i) {
        gpccrng::u64x4 x = gpccrng::philox4x64(ctr[i][0], ctr[i][1], ctr[i][2], ctr[i][3], key[i][0], key[i][1]);
        printf("W %llu %llu %llu %llu\n", (unsigned long long)x.v[0], (unsigned long long)x.v[1], (unsigned long long)x.v[2],
               (unsigned long long)x.v[3]);
    }
    for (unsigned long long s = 0; s < 6; ++s)
        for (unsigned long long b = 0; b < 5; ++b) {
            double z[4];
            gpccrng::normal4(99, b, s, s == 5 ? ~0ULL : 2, z);
            printf("Z %.17g %.17g %.17g %.17g\n", z[0], z[1], z[2], z[3]);
        }
    std::vector<std::vector<double>> ws = {{1.0, 2.0, 3.0}, {0.0, 0.0, 5.0, 0.0}, {0.0, 1.0, 0.0, 1.0, 0.0}, {0.25, 0.25, 0.25, 0.25},
                                           {1e-300, 1.0, 1e-300}, {7.0}};
    for (auto &w : ws) {
        std::vector<double> c(w.size());
        double a = 0.0;
        for (size_t m = 0; m < w.size(); ++m) { a += w[m]; c[m] = a; }
        printf("R");
        for (unsigned long long s = 0; s < 2000; ++s) printf(" %d", gpccrng::pick_row(31, s, c.data(), w.data(), (int)w.size()));
        printf("\n");
    }
    return 0;
}
'''
WEIGHTS = [[1.0, 2.0, 3.0], [0.0, 0.0, 5.0, 0.0], [0.0, 1.0, 0.0, 1.0, 0.0], [0.25, 0.25, 0.25, 0.25], [1e-300, 1.0, 1e-300], [7.0]]


def test_header_matches_mirror(tmp_path):
    src, exe = tmp_path / "rng_check.cpp", str(tmp_path / "rng_check")
    src.write_text(_CPP)
    cc = subprocess.run(["g++", "-std=c++17", "-O2", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines()
    W = [[int(v) for v in l.split()[1:]] for l in out if l.startswith("W")]
    ctr = [[0, 0, 0, 0], [5, 7, 9, 11], [3, 2, 2**64 - 1, 1], [2**64 - 1] * 4]
    key = [[0, 0], [123, 456], [42, 0], [2**64 - 1, 1]]
    for w, c, k in zip(W, ctr, key):
        assert w == [int(v) for v in rng.philox4x64(c, k)], (c, k)
    Z = np.array([[float(v) for v in l.split()[1:]] for l in out if l.startswith("Z")]).reshape(6, 20)
    for s in range(6):
        ref = rng.normals(99, 20, [s], rng.MIXROW if s == 5 else 2)[0]
        assert np.all(np.abs(Z[s] - ref) <= 1e-15 * np.maximum(1.0, np.abs(ref))), s
    R = [np.array([int(v) for v in l.split()[1:]]) for l in out if l.startswith("R")]
    for r, w in zip(R, WEIGHTS):
        ref = rng.pick_rows(31, 2000, w)
        assert np.array_equal(r, ref), w
        assert np.all(np.asarray(w)[r] > 0)                         # never a zero-weight row
        freq = np.bincount(r, minlength=len(w)) / 2000.0
        p = np.asarray(w) / np.sum(w)
        assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / 2000) + 1e-12), (w, freq)


def test_pick_rows_ties():
    """u c_{M-1} exactly on a cumulative weight goes to the next row (the first m with x < c_m)."""
    u = rng.pick_uniforms(5, 64)
    w = np.array([1.0, 1.0])
    c = rng.cumulative_weights(w)
    r = rng.pick_rows(5, 64, w)
    assert np.array_equal(r, (u * c[-1] >= c[0]).astype(np.int32))


def _case(Nl, Nt, seed):
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    r = np.random.default_rng(seed)
    span = max(float(np.max(a)) for a in t)
    tt = [np.sort(r.random(n) * (span + 10) - 5) for n in Nt]
    st = [0.05 + 0.2 * r.random(n) for n in Nt]
    return t, y, s, tt, st


@pytest.mark.parametrize("slip", ["no_jitter", "transpose", "no_bbar", "shift", "no_b_cross"])
def test_bar_rejects_slips(oracle, slip):
    """Each slip lands far above the bar max(1e-10, 64 eps cond_1(K_aug)) max(1, max |f*|).  (no_jitter: the latent curve, sigma* =
    0, of the fixed-b OU model, where the 1e-8 is what keeps the test block off singular.)"""
    t, y, s, tt, st = _case([180, 150], [40, 33], seed=11)
    kname, mb = "matern32", True
    if slip == "no_jitter":
        kname, mb, st = "OU", False, None
    T = sum(len(a) for a in tt)
    z = rng.normals(3, T, np.arange(8), 0)
    ref, cond = SW.draws(oracle, kname, t, y, s, [0.0, 2.0], [1.1, 0.8], 2.5, tt, st, z, mb)
    d2, _ = SW.draws(oracle, kname, t, y, s, [0.0, 2.0], [1.1, 0.8], 2.5, tt, st, z, mb, slip=slip)
    ratio = np.max(np.abs(d2 - ref)) / SW.bar(cond, ref)
    print("%s: error / bar %.3g (cond_1(K_aug) %.3g)" % (slip, ratio, cond))
    assert ratio > 10.0, (slip, ratio)
