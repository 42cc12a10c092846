"""Test infrastructure: the parity suite's comparisons of two renders (films and work counters) and of two sets of ray hits.

What is compared is every field of PtCounters but `wavefront_stages` (the device's own schedule; the oracle leaves it 0), and, in the
production walk, but the node counter (conftest.ckeys). A counter added to PtCounters is compared everywhere without a list to edit."""
import os

import numpy as np
from conftest import ckeys

ORACLE_THREADS = min(16, os.cpu_count() or 1)   # a GPU job has 16 CPUs; os.cpu_count() reports the whole machine's


def compared_counters():
    from _pkg import import_pkg
    return ckeys(name for name, _ in import_pkg()._abi.PtCounters._fields_ if name != "wavefront_stages")


def _plain(v):
    return [int(x) for x in v] if np.ndim(v) else int(v)


def assert_same_counters(got, want, skip=None):
    """got == want over compared_counters(); `skip` {name: reason} leaves out the counters it names, each for the reason given."""
    skip = skip or {}
    names = compared_counters()
    assert set(skip) <= set(names), sorted(set(skip) - set(names))
    for k in names:
        if k not in skip:
            assert _plain(got[k]) == _plain(want[k]), "counter %s: %s != %s" % (k, _plain(got[k]), _plain(want[k]))


def assert_same_film(film, ref, rtol=2e-6, atol=1e-7, weights="exact", resolved=None):
    """Weight channel bit for bit, or within relative tolerance `weights` (filters whose splats overlap: float atomics reorder the sums); radiance
    within rtol / atol; resolved=(resolve_got, resolve_want, max_abs) also bounds the resolved images' largest absolute difference."""
    if weights == "exact":
        assert np.array_equal(film[..., 3], ref[..., 3]), "weights differ"
    else:
        np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=weights, atol=0)
    np.testing.assert_allclose(film[..., :3], ref[..., :3], rtol=rtol, atol=atol)
    if resolved is not None:
        resolve_got, resolve_want, max_abs = resolved
        assert np.abs(resolve_got(film) - resolve_want(ref)).max() < max_abs


def assert_same_render(film, ref, got_counters, want_counters, skip=None, **film_kw):
    assert_same_counters(got_counters, want_counters, skip)
    assert_same_film(film, ref, **film_kw)


def assert_render_matches_oracle(pkg, gpu, oracle, sd, rp, nthreads=4, resolved=1e-4, skip=None, **film_kw):
    """One render of (sd, rp) on the GPU and one on the oracle: every counter, the film, the resolved images within `resolved` (None: not compared).
    Returns (film, ref, gpu_counters, oracle_counters)."""
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    film = g.render(rp)
    ref = orc.render(rp, nthreads=nthreads)
    gc, oc = g.counters(), orc.counters()
    assert_same_render(film, ref, gc, oc, skip, resolved=None if resolved is None else (g.resolve, orc.resolve, resolved), **film_kw)
    return film, ref, gc, oc


def assert_same_hits(got, want, got_counters, want_counters, skip=None):
    """trace_closest results (prim, t, b) -- prim equal, t and b bit for bit -- or trace_any hit flags, then every counter."""
    if isinstance(got, tuple):
        (gp, gt, gb), (wp, wt, wb) = got, want
        assert np.array_equal(gp, wp), "prims differ"
        assert np.array_equal(gt.view(np.uint32), wt.view(np.uint32)), "t differs"
        assert np.array_equal(gb.view(np.uint32), wb.view(np.uint32)), "b differs"
    else:
        assert np.array_equal(got, want), "hits differ"
    assert_same_counters(got_counters, want_counters, skip)
