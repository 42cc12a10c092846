"""VertexQueues' ray queue (kern_shade_common.h) on its own, through pt_test_ray_queue_push: a kernel that instantiates VertexQueues as k_shade, k_bssrdf and
k_shade_medium do -- init, per round one push per thread and flush(job, 256, false), at the end flush(job, 0, true) -- with the ray kinds of every thread-round
given by the host (bit 0 continuation, bit 1 MIS, bit 2 shadow; the thread-round's number is its path id).

Checked: the ray queue holds exactly the (path id, kind) pairs pushed and its counter their number; a thread-round's entries are consecutive and in kind
order (what lets the mixed traversal launch trace a vertex's rays side by side); the continuation queue holds exactly the continuation ids.
Shapes: one and three blocks; one round (no mid-loop flush) and nine (all ones: the QCAP = 1024 continuation queue stands exactly at its threshold after round 3
and is exactly full after round 4; the ray queues flush after every round (768 and 1024 entries) or every second one (2048)); every QCAP the shade kernels use.
"threshold" is the ray queue's own boundary at QCAP = 1024: 768 + 512 entries leave exactly the 768-entry reserve, so no flush, and the next round fills the
queue to its last slot."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KIND_SHIFT, PID_MASK = 30, (1 << 30) - 1


def _masks(name, n_blocks, rounds):
    n = n_blocks * rounds * 256
    m = np.zeros(n, np.uint8)
    if name == "ones":
        m[:] = 7
    elif name == "lane63_of_the_last_wave":
        m[n - 1] = 7
    elif name == "eight_combinations_in_one_wave":
        m[64:128] = np.arange(64) % 8
    elif name == "random":
        m[:] = np.random.default_rng(n).integers(0, 8, n)
    elif name == "threshold":
        m[:] = 7
        if rounds > 1:
            m[256:512] = 3          # block 0, round 1: two entries a thread
    else:
        assert name == "zeros"
    return m


@pytest.mark.parametrize("rounds", [1, 9])
@pytest.mark.parametrize("n_blocks", [1, 3])
@pytest.mark.parametrize("qcap", [256, 512, 1024])
def test_ray_queue_holds_each_vertex_rays_side_by_side(gpu, qcap, n_blocks, rounds):
    n = n_blocks * rounds * 256
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    for name in ("zeros", "ones", "lane63_of_the_last_wave", "eight_combinations_in_one_wave", "random", "threshold"):
        m = _masks(name, n_blocks, rounds)
        rays = np.full(3 * n, 0xFFFFFFFF, np.uint32); ext = np.full(n, 0xFFFFFFFF, np.uint32)
        n_rays, n_ext = C.c_uint32(), C.c_uint32()
        st = gpu.lib.pt_test_ray_queue_push(qcap, n_blocks, rounds, m.ctypes.data_as(u8p), rays.ctypes.data_as(u32p), C.byref(n_rays), ext.ctypes.data_as(u32p), C.byref(n_ext))
        assert st == 0, (name, st)
        t = np.arange(n, dtype=np.uint32)
        want = np.sort(np.concatenate([t[(m >> k) & 1 == 1] | np.uint32(k << KIND_SHIFT) for k in range(3)]))
        assert n_rays.value == len(want), (name, n_rays.value, len(want))
        got = rays[:n_rays.value]
        assert np.array_equal(np.sort(got), want), name
        assert (rays[n_rays.value:] == 0xFFFFFFFF).all(), name
        pid, kind = got & PID_MASK, got >> KIND_SHIFT
        same = pid[1:] == pid[:-1]
        assert (kind[1:][same] > kind[:-1][same]).all(), name                              # within a thread-round: kind order
        assert 1 + int((~same).sum()) == len(np.unique(pid)) or len(got) == 0, name     # ... and one run per thread-round: its entries are consecutive
        assert n_ext.value == int((m & 1).sum()), name
        assert np.array_equal(np.sort(ext[:n_ext.value]), t[m & 1 == 1]), name
