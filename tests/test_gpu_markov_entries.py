"""The frame the nine linear-time value and derivative entries share ("The host driver"), as a table: one row per
entry, every test over every row -- the argument checks and their order, M = 0, the counter, a NULL block, what a longer chain returns
bitwise of a shorter one, and the handle flavours.  The raw symbols, since the Python wrapper cannot pass a NULL pointer or M = -1.
A tenth entry is one more row of ENTRIES."""
from collections import namedtuple

import numpy as np
import pytest

import _markov_cases as MC
import gpcc_amd
from gpcc_amd import _capi
from gpcc_amd.api import _dp, _ip

pytestmark = pytest.mark.gpu

ARGUMENT, UNSUPPORTED = -1, -3
M, L = 5, 2

# symbol; noise: takes kappa and nu; grad: the gradient row's width (None: no gradient); block: the block's order (None: no block);
# counts: a good call adds M to markov_count; dense: the dense entry a refusal names
Entry = namedtuple("Entry", "symbol noise grad block counts dense")
ENTRIES = [
    Entry("gpcc_loglik_markov_batch", False, None, None, True, "gpcc_loglik_batch"),
    Entry("gpcc_loglik_grad_markov_batch", False, 2 * L + 1, None, False, "gpcc_loglik_grad_batch"),
    Entry("gpcc_loglik_hess_hyper_markov_batch", False, 2 * L + 1, L + 1, False, "gpcc_loglik_hess_hyper_batch"),
    Entry("gpcc_loglik_hess_markov_batch", False, 2 * L + 1, 2 * L + 1, False, "gpcc_loglik_hess_batch"),
    Entry("gpcc_loglik_fisher_markov_batch", False, 2 * L + 1, 2 * L + 1, False, "gpcc_loglik_hess_batch"),
    Entry("gpcc_loglik_noise_markov_batch", True, None, None, True, "gpcc_loglik_batch"),
    Entry("gpcc_loglik_grad_noise_markov_batch", True, 4 * L + 1, None, True, "gpcc_loglik_grad_batch"),
    Entry("gpcc_loglik_hess_noise_markov_batch", True, 4 * L + 1, 3 * L + 1, True, "gpcc_loglik_hess_hyper_batch"),
    Entry("gpcc_loglik_hess_full_noise_markov_batch", True, 4 * L + 1, 4 * L + 1, True, "gpcc_loglik_hess_batch"),
]
VALUE = {False: "gpcc_loglik_markov_batch", True: "gpcc_loglik_noise_markov_batch"}            # a family's value entry
GRADIENT = {False: "gpcc_loglik_grad_markov_batch", True: "gpcc_loglik_grad_noise_markov_batch"}   # ... and its gradient entry
REQUIRED = ("delays", "alpha", "rho", "loglik", "grad", "info")
entries = pytest.mark.parametrize("e", ENTRIES, ids=[e.symbol for e in ENTRIES])


def _rows():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    rg = np.random.default_rng(5)
    rows = {"delays": np.ascontiguousarray(d0 + rg.uniform(-0.5, 0.5, (M, L))), "alpha": rg.uniform(0.4, 2.0, (M, L)),
            "rho": np.exp(rg.uniform(np.log(0.5), np.log(30.0), M)), "kappa": rg.uniform(0.5, 2.0, (M, L)),
            "nu": rg.uniform(0.0, 0.05, (M, L))}
    return (t, y, s), rows


DATA, ROWS = _rows()


def call(h, e, m=M, null=()):
    """The raw entry on handle h (None: NULL) with m rows; null: the arguments passed as NULL ("all": every pointer).  -> (rc, the
    arrays by name); an array the call did not write keeps -7."""
    out = {"loglik": np.full(M, -7.0), "info": np.full(M, -7, np.int32)}
    if e.grad:
        out["grad"] = np.full((M, e.grad), -7.0)
    if e.block:
        out["block"] = np.full((M, e.block, e.block), -7.0)
    names = ["delays", "alpha", "rho"] + (["kappa", "nu"] if e.noise else []) + ["loglik"] + [n for n in ("grad", "block") if n in out]
    args = [None if null == "all" or n in null else _dp(ROWS[n] if n in ROWS else out[n]) for n in names]
    rc = getattr(_capi.load(), e.symbol)(h, m, *args, None if null == "all" or "info" in null else _ip(out["info"]))
    return rc, out


def same(x, z, names=None):
    return all(np.array_equal(x[n], z[n], equal_nan=True) for n in (names or z))


@pytest.fixture(scope="module")
def handles():
    """One handle per flavour on matern32 and on rbf, and the fp64 single-device handle's arrays of every entry with what the call
    added to markov_count."""
    flavours = {"fp64": {}, "fp32": {"precision": "fp32"}, "two devices": {"devices": [0, 0]}}
    objs = {(k, f): gpcc_amd.Objective(*DATA, getattr(gpcc_amd, k), **kw) for k in ("matern32", "rbf") for f, kw in flavours.items()}
    good, added = {}, {}
    obj = objs["matern32", "fp64"]
    for e in ENTRIES:
        before = obj.get_option("markov_count")
        rc, good[e.symbol] = call(obj._h, e)
        assert rc == 0, (e.symbol, _capi.last_error(obj._h))
        added[e.symbol] = obj.get_option("markov_count") - before
    yield objs, good, added
    for o in objs.values():
        o.close()


@entries
def test_null_handle_and_negative_m(handles, e):
    objs, _, _ = handles
    rc, _ = call(None, e)
    assert rc == ARGUMENT and _capi.last_error(None) == "NULL handle"
    h = objs["matern32", "fp64"]._h
    rc, _ = call(h, e, m=-1)
    assert rc == ARGUMENT and "M=-1 < 0" in _capi.last_error(h)


@entries
def test_no_rows_before_any_pointer(handles, e):
    objs, _, _ = handles
    rc, _ = call(objs["matern32", "fp64"]._h, e, m=0, null="all")
    assert rc == 0


@entries
def test_each_required_pointer(handles, e):
    """delays, alpha, rho, loglik, info and, where the entry has one, grad: NULL is refused before any work, and the handle is as good
    as before.  kappa and nu NULL are no errors (all 1, all 0)."""
    objs, good, _ = handles
    obj = objs["matern32", "fp64"]
    for name in REQUIRED:
        if name == "grad" and not e.grad:
            continue
        before = obj.get_option("markov_count")
        rc, out = call(obj._h, e, null=(name,))
        assert rc == ARGUMENT and _capi.last_error(obj._h) == "NULL pointer", name
        assert obj.get_option("markov_count") == before, name
        assert all((x == -7).all() for x in out.values()), name
        rc, out = call(obj._h, e)
        assert rc == 0 and same(out, good[e.symbol]), name
    if e.noise:
        rc, out = call(obj._h, e, null=("kappa", "nu"))
        assert rc == 0 and (out["info"] == 0).all() and np.isfinite(out["loglik"]).all()


@entries
def test_counter(handles, e):
    _, _, added = handles
    assert added[e.symbol] == (M if e.counts else 0)


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.block], ids=[e.symbol for e in ENTRIES if e.block])
def test_null_block_is_the_gradient_entry(handles, e):
    objs, good, _ = handles
    rc, out = call(objs["matern32", "fp64"]._h, e, null=("block",))
    assert rc == 0 and same(out, good[GRADIENT[e.noise]]) and (out["block"] == -7).all()


@entries
def test_chain_identities(handles, e):
    _, good, _ = handles
    out = good[e.symbol]
    assert (out["info"] == 0).all() and all(np.isfinite(x).all() for x in out.values())
    assert same(out, good[VALUE[e.noise]], ("loglik", "info"))
    if e.grad:
        assert same(out, good[GRADIENT[e.noise]], ("grad",))
    if e.symbol == "gpcc_loglik_hess_markov_batch":
        assert np.array_equal(out["block"][:, :L + 1, :L + 1], good["gpcc_loglik_hess_hyper_markov_batch"]["block"], equal_nan=True)
    if e.symbol == "gpcc_loglik_hess_full_noise_markov_batch":
        idx = np.r_[0:L + 1, 2 * L + 1:4 * L + 1]
        assert np.array_equal(out["block"][:, idx][:, :, idx], good["gpcc_loglik_hess_noise_markov_batch"]["block"], equal_nan=True)


@entries
@pytest.mark.parametrize("flavour", ["fp32", "two devices"])
def test_handle_flavours(handles, e, flavour):
    objs, good, _ = handles
    rc, out = call(objs["matern32", flavour]._h, e)
    assert rc == 0 and same(out, good[e.symbol])


@entries
@pytest.mark.parametrize("flavour", ["fp64", "fp32", "two devices"])
def test_rbf_is_refused_under_the_entrys_name(handles, e, flavour):
    objs, _, _ = handles
    h = objs["rbf", flavour]._h
    rc, out = call(h, e)
    msg = _capi.last_error(h)
    assert rc == UNSUPPORTED and msg.startswith(e.symbol + ": ") and "use " + e.dense in msg, msg
    assert all((x == -7).all() for x in out.values())
