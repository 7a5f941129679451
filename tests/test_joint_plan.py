"""CPU: the joint draw's launch plan (plan_joint_draw, csrc/joint_plan.hpp) through gpmpc_debug_joint_plan, for the closed loops'
shapes and the paths the knobs select.  Each expected line is the kernel sequence the dispatcher launched for the same call before
it was split into a plan and an executor (kernel trace of that build; one batch's steps, repeated `batches` times, then the eigh
launches).  The rows of the cache-hit oracle comparisons (small batches behind a hit cache, a covariance-only repeat, a prefix cache) are
read off plan_joint_draw's branches instead; the GPU tests that make those calls assert the steps named there on the call's own plan."""
import ctypes

import pytest

from sampling_gpmpc_amd import _lib

# (g_ny, T, N_r): the car (45 real points, value + two derivatives), the pendulum (36 real points), the car's value-only model
CAR, PEND, CAR_T1 = (3, 3, 45), (1, 3, 36), (3, 1, 45)
# (g_ny, T, N_r, real_has_grad): the boundaries of the real block - 64 / 65 observed real slots, value-only (n_r = N_r) and with gradient
# labels (n_r = 3 N_r: 63 / 66)
PEND_64, PEND_65, PEND_21G, PEND_22G = (1, 3, 64), (1, 3, 65), (1, 3, 21, True), (1, 3, 22, True)

# (desc, Ns, n_h, n_ho, m, cache_rows (0: no caller cache), n_cached, pending, root_mode, eigh rank hint, knob, expected line)
PLANS = [
    # car 1024 x 40, MPC step 0, k = 0
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma(abandon) | eigh=narrow+deferred pending_written=0'),
    # k = 1
    (CAR, 1024, 40, 120, 40, 512, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # k = 2
    (CAR, 1024, 80, 240, 40, 512, 120, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # k = 3
    (CAR, 1024, 120, 360, 40, 512, 240, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # MPC step 1, k = 0: 45 + 480 slots, TOP / BOTTOM
    (CAR, 1024, 160, 480, 40, 512, 360, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma(abandon) | eigh=narrow+deferred pending_written=0'),
    # car 4096 x 40, k = 0
    (CAR, 4096, 0, 0, 40, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma(abandon) | eigh=narrow+deferred pending_written=0'),
    # k = 1
    (CAR, 4096, 40, 120, 40, 512, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # k = 2
    (CAR, 4096, 80, 240, 40, 512, 120, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # k = 3
    (CAR, 4096, 120, 360, 40, 512, 240, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # pendulum 1024 x 30, k = 0
    (PEND, 1024, 0, 0, 30, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # k = 1: 90 slots, m T = 90 - the matrix pipe
    (PEND, 1024, 30, 90, 30, 256, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # car H = 20, k = 1: 60 slots, narrow test block - the VALU path
    (CAR, 1024, 20, 60, 20, 256, 0, 2, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=121) joint_tail_mfma(abandon) | eigh=narrow+deferred pending_written=0'),
    # value-only model (T = 1): one launch
    (CAR_T1, 1024, 0, 0, 40, 0, 0, 0, 0, 0, '',
     'path=1 batches=1 | joint_kernel(ALL,nrow=41) | eigh=narrow+deferred pending_written=0'),
    # gpmpc_debug_eigh_narrow(0)
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 0, 100, 'narrow=0',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # gpmpc_debug_eigh_narrow(1)
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 0, 0, 'narrow=1',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma(abandon) | eigh=narrow+deferred pending_written=0'),
    # eigh rank hint above the narrow cap
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 0, 100, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # gpmpc_debug_joint_real_kernel(0), k = 0
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 0, 100, 'real=0',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=121) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # gpmpc_debug_joint_real_kernel(0), k = 1
    (CAR, 1024, 40, 120, 40, 384, 0, 2, 0, 100, 'real=0',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=full pending_written=1'),
    # gpmpc_debug_joint_real_kernel(1), k = 1
    (CAR, 1024, 40, 120, 40, 384, 0, 2, 0, 100, 'real=1',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(abandon,Sv=cache) | eigh=full pending_written=1'),
    # GPMPC_ROOT_CHOLESKY: no eigh step
    (CAR, 1024, 0, 0, 40, 0, 0, 0, 2, 100, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma() | eigh=none pending_written=0'),
    # the VALU path pinned
    (CAR, 1024, 40, 120, 40, 384, 0, 2, 0, 100, 'pin=1',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=241) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # no caller cache, nothing cached: three temporary-cache batches
    (CAR, 1024, 40, 120, 40, 0, 0, 0, 0, 100, '',
     'path=2 batches=3 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # no caller cache, more new rows than test slots: joint_kernel FACTOR first
    (CAR, 1024, 80, 240, 40, 0, 0, 0, 0, 100, '',
     'path=2 batches=3 | joint_kernel(FACTOR,nrow=240) joint_test_mfma(TEST) joint_tail_mfma(abandon) | eigh=full pending_written=0'),
    # m T = 135 > 128: the VALU path in one launch
    (CAR, 256, 45, 135, 45, 384, 0, 2, 0, 100, '',
     'path=1 batches=1 | joint_kernel(ALL,nrow=271) | eigh=full pending_written=0'),
    # (new rows go to the END of the table: a row's position is part of its test id)
    # the calls of the cache-hit oracle comparisons (tests/test_hip_parity.py, tests/test_hip_joint_cache_parity.py)
    # pendulum 16 x 30, k = 2 with pending rows: the in-place Cholesky of the block the k = 1 draw left, nothing else in front of the test rows
    (PEND, 16, 60, 180, 30, 384, 90, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # the same call allowed to WRITE pending rows only (the previous draw left none): the new rows against the cached columns
    (PEND, 16, 60, 180, 30, 384, 90, 2, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # ... and with pending rows off (GPMPC_JOINT_PENDING=0)
    (PEND, 16, 60, 180, 30, 384, 90, 0, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # a covariance-only repeat of that posterior (every row cached): no factor step, the pending rows are written again
    (PEND, 16, 60, 180, 30, 384, 180, 2, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # pendulum 6 x 30, k = 5: 36 + 450 = 486 slots, TOP / BOTTOM behind 360 cached rows and a pending block
    (PEND, 6, 150, 450, 30, 640, 360, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # ... with pending rows off
    (PEND, 6, 150, 450, 30, 640, 360, 0, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # pendulum, MPC step 1, k = 0 behind a 384-row cache: 396 slots in one launch, no room for pending rows behind the 360 slots
    (PEND, 16, 120, 360, 30, 384, 270, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # a cache that holds a prefix of the samples (3 of 7), k = 2: the cached samples without pending rows ...
    (PEND, 3, 60, 180, 30, 384, 90, 0, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # ... and the other four through the workspace's temporary cache
    (PEND, 4, 60, 180, 30, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_kernel(FACTOR,nrow=180) joint_test_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # the boundaries of the real block (tests/joint_variants.py runs them on the device).  64 observed real slots: the matrix pipe, k = 0,
    # 1, 2 of the pendulum 16 x 30 ...
    (PEND_64, 16, 0, 0, 30, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_64, 16, 30, 90, 30, 256, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    (PEND_64, 16, 60, 180, 30, 384, 90, 3, 0, 0, '',
     'path=2 batches=1 | joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # ... and a narrow test block with the matrix pipe pinned
    (PEND_64, 16, 12, 36, 12, 256, 0, 2, 0, 0, 'pin=2',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # 65: no matrix-pipe kernel takes the real block - the VALU path at every k (90 rows cached at k = 2), also with the matrix pipe pinned
    (PEND_65, 16, 0, 0, 30, 0, 0, 0, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=91) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_65, 16, 30, 90, 30, 256, 0, 2, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=181) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_65, 16, 60, 180, 30, 384, 90, 3, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=181) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_65, 16, 12, 36, 12, 256, 0, 2, 0, 0, 'pin=2',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=73) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # gradient labels on the real data: 21 points are 63 observed slots (the matrix pipe; k = 2 with pending rows off) ...
    (PEND_21G, 16, 0, 0, 30, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_21G, 16, 30, 90, 30, 256, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    (PEND_21G, 16, 60, 180, 30, 384, 90, 0, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # ... 22 points are 66
    (PEND_22G, 16, 0, 0, 30, 0, 0, 0, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=91) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_22G, 16, 30, 90, 30, 256, 0, 2, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=181) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_22G, 16, 60, 180, 30, 384, 90, 0, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=181) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    # the pair tables of joint_real_mfma_kernel (36 KB): 64 real points against m = 41 test points fit (36,128 B), k = 0 and 1 ...
    (PEND_64, 3, 0, 0, 41, 0, 0, 0, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(TEST) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_64, 3, 41, 123, 41, 256, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
    # ... against 42 they do not (37,320 B): the VALU head at k = 0, joint_test_mfma_kernel's factor mode at k = 1
    (PEND_64, 3, 0, 0, 42, 0, 0, 0, 0, 0, '',
     'path=1 batches=1 | joint_kernel(HEAD,nrow=127) joint_tail_mfma() | eigh=narrow+deferred pending_written=0'),
    (PEND_64, 3, 42, 126, 42, 256, 0, 2, 0, 0, '',
     'path=2 batches=1 | joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache) | eigh=narrow+deferred pending_written=1'),
]


def _raw():
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.gpmpc_debug_joint_plan.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 8 + [ctypes.c_char_p, ctypes.c_size_t]
    return raw


@pytest.mark.parametrize("desc,Ns,n_h,n_ho,m,cache_rows,n_cached,pending,root_mode,rank,knob,expected", PLANS)
def test_joint_plan(desc, Ns, n_h, n_ho, m, cache_rows, n_cached, pending, root_mode, rank, knob, expected):
    raw = _raw()
    g_ny, T, N_r, *has_grad = desc                              # (a fourth field: real_has_grad)
    d = _lib.make_gp_desc(g_ny, 2, T, N_r, bool(has_grad and has_grad[0]), [[2.0, 1.1]] * g_ny, [0.05] * g_ny, [2e-7] * T, 1e-20)
    name, _, val = knob.partition("=")
    setters = {"pin": (raw.gpmpc_joint_pin_path, 0), "narrow": (raw.gpmpc_debug_eigh_narrow, -1),
               "real": (raw.gpmpc_debug_joint_real_kernel, -1)}
    if name:
        setters[name][0](int(val))
    try:
        buf = ctypes.create_string_buffer(512)
        rc = raw.gpmpc_debug_joint_plan(ctypes.addressof(d), Ns, n_h, n_ho, m, cache_rows, n_cached, pending, root_mode, rank, buf, 512)
    finally:
        if name:
            setters[name][0](setters[name][1])
    assert rc == 0
    assert buf.value.decode() == expected
