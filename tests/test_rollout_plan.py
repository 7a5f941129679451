"""CPU: the rollout's launch plan (plan_rollout_launch, csrc/rollout_plan.hpp) through gpmpc_debug_rollout_plan, for the shapes,
sizes, knobs and pins that select each kernel.  Each expected line is what the dispatcher launched for the same call before it was
split into a plan and an executor: that build's launchers, made to report their instance, grid, block, LDS, workspace check and
RolloutArgs layout instead of launching.  The workspace queries are pinned to that build's values."""
import ctypes
import re

import pytest

from sampling_gpmpc_amd import _lib

R, I = _lib.MODE_RECONDITIONED, _lib.MODE_INDEPENDENT
# (g_ny, T, N_r, real_has_grad, grid): the pendulum (4 x 9 grid) and the car (5 x 9), their one-size-up grids, the value-only
# models, real data with derivatives, real inputs off the grid
PEND, CAR = (1, 3, 36, False, (4, 9)), (3, 3, 45, False, (5, 9))
PEND59, CAR69 = (1, 3, 45, False, (5, 9)), (3, 3, 54, False, (6, 9))
PEND_T1, CAR_T1 = (1, 1, 36, False, (4, 9)), (3, 1, 45, False, (5, 9))
PEND_GRAD, PEND_NOGRID = (1, 3, 36, True, (4, 9)), (1, 3, 36, False, (0, 0))
KERNELS = {"rollout_kernel": _lib.KERNEL_GENERIC, "rollout_fast_kernel": _lib.KERNEL_FAST, "rollout_indep_kernel": _lib.KERNEL_INDEP,
           "rollout_indep_grid_kernel": _lib.KERNEL_INDEP, "rollout_tiles_kernel": _lib.KERNEL_TILES, "rollout_one_kernel": _lib.KERNEL_ONE}

# (desc, mode, hall_tasks, Ns, H, n_h0, n_v0, state_slots (0: no factor state), state_points, knobs / pin, expected line)
PLANS = [
    # configs[1] (the bench's shape): the one-chain kernel
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, '',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=1024 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    # up to 2048 chains the one-chain kernel ...
    (PEND, R, 3, 2048, 30, 0, 0, 0, 0, '',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=2048 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    # ... from 2049 on the tiled one
    (PEND, R, 3, 2049, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=513 block=64 lds=40768 ws=138682368 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=1024 block=64 lds=40768 ws=276824064 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 16384, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=4096 block=64 lds=40768 ws=1107296256 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    # 3 (H - 1) > 88: beyond the one-chain kernel; the tuned kernel up to 1024 chains ...
    (PEND, R, 3, 1024, 40, 0, 0, 0, 0, '',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=0,GRID=1> grid=256 block=256 lds=69440 ws=56296448 zero=1 | nh_max=117 lds_shared=0 lds_per_wave=2170 linv_in_lds=1 ws_chain_stride=6872 max_points=40'),
    # ... the tiled one above
    (PEND, R, 3, 1025, 40, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=257 block=64 lds=51648 ws=69476352 zero=0 | nh_max=117 lds_shared=170 lds_per_wave=13018 linv_in_lds=1 ws_chain_stride=33792 max_points=40'),
    # 3 (H - 1) > 128: beyond the tuned kernel: the tiled one with 40 tile rows
    (PEND, R, 3, 1024, 50, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=40,SEED=0> grid=256 block=64 lds=62528 ws=107479040 zero=0 | nh_max=147 lds_shared=210 lds_per_wave=18162 linv_in_lds=1 ws_chain_stride=52480 max_points=50'),
    (PEND, R, 3, 1024, 2, 0, 0, 0, 0, '',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=1024 block=64 lds=5280 ws=0 zero=0 | nh_max=3 lds_shared=18 lds_per_wave=1674 linv_in_lds=1 ws_chain_stride=114 max_points=2'),
    # H = 1: no kernel but the generic one
    (PEND, R, 3, 1024, 1, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=1> grid=1024 block=64 lds=12832 ws=0 zero=0 | nh_max=1 lds_shared=14 lds_per_wave=1590 linv_in_lds=1 ws_chain_stride=37 max_points=1'),
    # car: the tuned kernel up to 768 chains ...
    (CAR, R, 3, 256, 40, 0, 0, 0, 0, '',
     'rollout_fast_kernel<T=3,NR=45,G_NY=3,ENV=car,LHH_LDS=0,GRID=1> grid=256 block=192 lds=63024 ws=42222592 zero=1 | nh_max=117 lds_shared=6 lds_per_wave=2624 linv_in_lds=1 ws_chain_stride=6872 max_points=40'),
    # ... the tiled one above
    (CAR, R, 3, 257, 40, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=32,SEED=0> grid=257 block=64 lds=40608 ws=69476352 zero=0 | nh_max=117 lds_shared=252 lds_per_wave=2694 linv_in_lds=1 ws_chain_stride=33792 max_points=40'),
    # car at 32 / 40 / 48 tile rows
    (CAR, R, 3, 4096, 40, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=32,SEED=0> grid=4096 block=64 lds=40608 ws=1107296256 zero=0 | nh_max=117 lds_shared=252 lds_per_wave=2694 linv_in_lds=1 ws_chain_stride=33792 max_points=40'),
    (CAR, R, 3, 4096, 50, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=40,SEED=0> grid=4096 block=64 lds=49248 ws=1719664640 zero=0 | nh_max=147 lds_shared=312 lds_per_wave=2784 linv_in_lds=1 ws_chain_stride=52480 max_points=50'),
    (CAR, R, 3, 4096, 60, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=48,SEED=0> grid=4096 block=64 lds=57888 ws=2466250752 zero=0 | nh_max=177 lds_shared=372 lds_per_wave=2874 linv_in_lds=1 ws_chain_stride=75264 max_points=60'),
    # no tuned alternative at 3 (H - 1) > 128: the tiled kernel from 256 chains on
    (CAR, R, 3, 256, 50, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=40,SEED=0> grid=256 block=64 lds=49248 ws=107479040 zero=0 | nh_max=147 lds_shared=312 lds_per_wave=2784 linv_in_lds=1 ws_chain_stride=52480 max_points=50'),
    (CAR, R, 3, 64, 40, 0, 0, 0, 0, '',
     'rollout_fast_kernel<T=3,NR=45,G_NY=3,ENV=car,LHH_LDS=0,GRID=1> grid=64 block=192 lds=63024 ws=10556416 zero=1 | nh_max=117 lds_shared=6 lds_per_wave=2624 linv_in_lds=1 ws_chain_stride=6872 max_points=40'),
    # the one-size-up grids: the tiled kernel with 32 tile rows ...
    (PEND59, R, 3, 1024, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=pendulum,NT=32,SEED=0> grid=256 block=64 lds=42624 ws=69206016 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=10348 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    # ... and no more
    (PEND59, R, 3, 1024, 50, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=4,FAC_LDS=0> grid=1024 block=64 lds=23952 ws=143302656 zero=0 | nh_max=147 lds_shared=210 lds_per_wave=2784 linv_in_lds=1 ws_chain_stride=17493 max_points=50'),
    (CAR69, R, 3, 1024, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=6,N1=9,ENV=car,NT=32,SEED=0> grid=1024 block=64 lds=33504 ws=276824064 zero=0 | nh_max=87 lds_shared=192 lds_per_wave=642 linv_in_lds=0 ws_chain_stride=33792 max_points=30'),
    (CAR69, R, 3, 1024, 40, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=6,N1=9,ENV=car,NT=32,SEED=0> grid=1024 block=64 lds=42144 ws=276824064 zero=0 | nh_max=117 lds_shared=252 lds_per_wave=732 linv_in_lds=0 ws_chain_stride=33792 max_points=40'),
    # no grid: the tuned kernel without the grid root
    (PEND_NOGRID, R, 3, 1024, 30, 0, 0, 0, 0, '',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=0> grid=256 block=256 lds=163776 ws=0 zero=0 | nh_max=87 lds_shared=1368 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    # mode I, value-only model: one sample per lane with the grid root
    (CAR_T1, I, 1, 262144, 40, 0, 0, 0, 0, '',
     'rollout_indep_grid_kernel<ENV=car,N0=5,N1=9,G_NY=3> grid=4096 block=192 lds=0 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2202 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (PEND_T1, I, 1, 4096, 30, 0, 0, 0, 0, '',
     'rollout_indep_grid_kernel<ENV=pendulum,N0=4,N1=9,G_NY=1> grid=64 block=64 lds=0 ws=0 zero=0 | nh_max=1 lds_shared=130 lds_per_wave=1436 linv_in_lds=1 ws_chain_stride=37 max_points=30'),
    # mode I with T = 3, and T = 1 in mode R: generic
    (CAR, I, 3, 1024, 40, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=0> grid=1024 block=192 lds=61104 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2462 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (CAR_T1, R, 1, 1024, 40, 0, 0, 0, 0, '',
     'rollout_kernel<T=1,RPL=1,FAC_LDS=1> grid=1024 block=192 lds=117552 ws=0 zero=0 | nh_max=39 lds_shared=252 lds_per_wave=4814 linv_in_lds=1 ws_chain_stride=2535 max_points=40'),
    # mode I beyond the generic sizing's LDS: rejected (its status comes first)
    (CAR_T1, I, 1, 1024, 2000, 0, 0, 0, 0, '',
     'error=-4 rollout: horizon too long for LDS vectors'),
    # real_has_grad: generic, RPL 1 / 2 / 4, the factor in LDS and (H = 60) in the workspace
    (PEND_GRAD, R, 3, 1024, 10, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=1> grid=1024 block=64 lds=33472 ws=0 zero=0 | nh_max=27 lds_shared=50 lds_per_wave=4134 linv_in_lds=0 ws_chain_stride=3294 max_points=10'),
    (PEND_GRAD, R, 3, 1024, 30, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=114992 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=14244 linv_in_lds=0 ws_chain_stride=13224 max_points=30'),
    (PEND_GRAD, R, 3, 1024, 60, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=4,FAC_LDS=0> grid=1024 block=64 lds=12320 ws=285646848 zero=0 | nh_max=177 lds_shared=250 lds_per_wave=1290 linv_in_lds=0 ws_chain_stride=34869 max_points=60'),
    # more than 256 slots per chain
    (PEND, R, 3, 1024, 100, 0, 0, 0, 0, '',
     'error=-4 rollout: more than 256 hallucinated label slots per chain'),
    # hall_tasks = 1: the tiled kernel (SEED) from 256 chains on
    (PEND, R, 1, 256, 30, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=1> grid=64 block=64 lds=40768 ws=17301504 zero=0 | nh_max=29 lds_shared=130 lds_per_wave=3176 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 1, 255, 30, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=1> grid=255 block=64 lds=26448 ws=0 zero=0 | nh_max=29 lds_shared=130 lds_per_wave=3176 linv_in_lds=1 ws_chain_stride=1479 max_points=30'),
    (CAR, R, 1, 86, 40, 0, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=32,SEED=1> grid=86 block=64 lds=40608 ws=23248896 zero=0 | nh_max=39 lds_shared=252 lds_per_wave=5074 linv_in_lds=1 ws_chain_stride=33792 max_points=40'),
    (CAR, R, 1, 85, 40, 0, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=1> grid=85 block=192 lds=123792 ws=0 zero=0 | nh_max=39 lds_shared=252 lds_per_wave=5074 linv_in_lds=1 ws_chain_stride=2535 max_points=40'),
    # seeded without a state: the tiled kernel from 256 chains on, generic below
    (PEND, R, 3, 256, 20, 5, 0, 0, 0, '',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=1> grid=64 block=64 lds=35328 ws=17301504 zero=0 | nh_max=72 lds_shared=100 lds_per_wave=6972 linv_in_lds=1 ws_chain_stride=33792 max_points=25'),
    (PEND, R, 3, 255, 20, 5, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=255 block=64 lds=56576 ws=0 zero=0 | nh_max=72 lds_shared=100 lds_per_wave=6972 linv_in_lds=1 ws_chain_stride=5220 max_points=25'),
    (CAR, R, 1, 86, 20, 0, 12, 0, 0, '',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=32,SEED=1> grid=86 block=64 lds=33696 ws=23248896 zero=0 | nh_max=31 lds_shared=156 lds_per_wave=4354 linv_in_lds=1 ws_chain_stride=33792 max_points=32'),
    # seeded, 3 (n_h0 + H - 1) > 192 rows: generic
    (PEND, R, 3, 1024, 30, 40, 0, 0, 0, '',
     'rollout_kernel<T=3,RPL=4,FAC_LDS=0> grid=1024 block=64 lds=18096 ws=237404160 zero=0 | nh_max=207 lds_shared=210 lds_per_wave=2052 linv_in_lds=1 ws_chain_stride=28980 max_points=70'),
    # a kept state, and a resume: generic, the factor in the state
    (PEND, R, 3, 1024, 20, 5, 0, 75, 25, '',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=0> grid=1024 block=64 lds=15184 ws=0 zero=0 | nh_max=75 lds_shared=140 lds_per_wave=1758 linv_in_lds=1 ws_chain_stride=5550 max_points=45'),
    (PEND, R, 3, 1024, 20, 0, 0, 120, 40, 'resume',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=0> grid=1024 block=64 lds=16144 ws=0 zero=0 | nh_max=120 lds_shared=170 lds_per_wave=1848 linv_in_lds=1 ws_chain_stride=11580 max_points=60'),
    # each knob on a shape it changes
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_ROLLOUT_ONE=0',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=1> grid=256 block=256 lds=152832 ws=0 zero=0 | nh_max=87 lds_shared=0 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'GPMPC_ROLLOUT_ONE=1',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=4096 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_ROLLOUT_TILES=1',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=256 block=64 lds=40768 ws=69206016 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'GPMPC_ROLLOUT_TILES=0',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=1> grid=1024 block=256 lds=152832 ws=0 zero=0 | nh_max=87 lds_shared=0 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_ROLLOUT_ONE=1,GPMPC_ROLLOUT_TILES=1',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=1024 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=4096 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (CAR_T1, I, 1, 262144, 40, 0, 0, 0, 0, 'GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_kernel<T=1,RPL=1,FAC_LDS=0> grid=262144 block=192 lds=54864 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2202 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=0> grid=256 block=256 lds=163776 ws=0 zero=0 | nh_max=87 lds_shared=1368 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=0> grid=1024 block=256 lds=163776 ws=0 zero=0 | nh_max=87 lds_shared=1368 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (CAR, R, 3, 256, 40, 0, 0, 0, 0, 'GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_fast_kernel<T=3,NR=45,G_NY=3,ENV=car,LHH_LDS=0,GRID=0> grid=256 block=192 lds=112704 ws=42222592 zero=1 | nh_max=117 lds_shared=6216 lds_per_wave=2624 linv_in_lds=1 ws_chain_stride=6872 max_points=40'),
    (CAR_T1, I, 1, 262144, 40, 0, 0, 0, 0, 'GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_indep_kernel<ENV=car,N0=5,N1=9,G_NY=3> grid=1024 block=256 lds=0 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2202 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=0,GRID=1> grid=256 block=256 lds=32960 ws=31212544 zero=1 | nh_max=87 lds_shared=0 lds_per_wave=1030 linv_in_lds=1 ws_chain_stride=3810 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=1024 block=64 lds=40768 ws=276824064 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=1812 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND_GRAD, R, 3, 1024, 10, 0, 0, 0, 0, 'GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_kernel<T=3,RPL=1,FAC_LDS=0> grid=1024 block=64 lds=7120 ws=26984448 zero=0 | nh_max=27 lds_shared=50 lds_per_wave=840 linv_in_lds=0 ws_chain_stride=3294 max_points=10'),
    # every pin
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=0',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=1> grid=256 block=256 lds=152832 ws=0 zero=0 | nh_max=87 lds_shared=0 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=2',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=3',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=256 block=64 lds=40768 ws=69206016 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'pin=4',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=4096 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 64, 30, 0, 0, 0, 0, 'pin=3',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=16 block=64 lds=40768 ws=4325376 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (CAR, R, 3, 4096, 40, 0, 0, 0, 0, 'pin=1',
     'rollout_fast_kernel<T=3,NR=45,G_NY=3,ENV=car,LHH_LDS=0,GRID=1> grid=4096 block=192 lds=63024 ws=675546112 zero=1 | nh_max=117 lds_shared=6 lds_per_wave=2624 linv_in_lds=1 ws_chain_stride=6872 max_points=40'),
    (CAR_T1, I, 1, 262144, 40, 0, 0, 0, 0, 'pin=0',
     'rollout_kernel<T=1,RPL=1,FAC_LDS=0> grid=262144 block=192 lds=54864 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2202 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (CAR_T1, I, 1, 262144, 40, 0, 0, 0, 0, 'pin=1',
     'rollout_indep_grid_kernel<ENV=car,N0=5,N1=9,G_NY=3> grid=4096 block=192 lds=0 ws=0 zero=0 | nh_max=1 lds_shared=252 lds_per_wave=2202 linv_in_lds=1 ws_chain_stride=46 max_points=40'),
    (PEND_T1, I, 1, 4096, 30, 0, 0, 0, 0, 'pin=3',
     'rollout_indep_grid_kernel<ENV=pendulum,N0=4,N1=9,G_NY=1> grid=64 block=64 lds=0 ws=0 zero=0 | nh_max=1 lds_shared=130 lds_per_wave=1436 linv_in_lds=1 ws_chain_stride=37 max_points=30'),
    (PEND, R, 3, 64, 20, 5, 0, 0, 0, 'pin=3',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=1> grid=16 block=64 lds=35328 ws=4325376 zero=0 | nh_max=72 lds_shared=100 lds_per_wave=6972 linv_in_lds=1 ws_chain_stride=33792 max_points=25'),
    (PEND, R, 3, 1024, 20, 5, 0, 0, 0, 'pin=4',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=56576 ws=0 zero=0 | nh_max=72 lds_shared=100 lds_per_wave=6972 linv_in_lds=1 ws_chain_stride=5220 max_points=25'),
    (PEND, R, 3, 1024, 20, 5, 0, 75, 25, 'pin=3',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=0> grid=1024 block=64 lds=15184 ws=0 zero=0 | nh_max=75 lds_shared=140 lds_per_wave=1758 linv_in_lds=1 ws_chain_stride=5550 max_points=45'),
    # precedence
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=1,GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=1> grid=256 block=256 lds=152832 ws=0 zero=0 | nh_max=87 lds_shared=0 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=4,GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=3,GPMPC_DISABLE_FAST_ROLLOUT=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=4,GPMPC_ROLLOUT_TILES=1',
     'rollout_one_kernel<N0=4,ENV=pendulum> grid=1024 block=64 lds=5280 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 4096, 30, 0, 0, 0, 0, 'pin=3,GPMPC_ROLLOUT_TILES=0',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=1024 block=64 lds=40768 ws=276824064 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=3,GPMPC_ROLLOUT_ONE=1',
     'rollout_tiles_kernel<N0=4,N1=9,ENV=pendulum,NT=32,SEED=0> grid=256 block=64 lds=40768 ws=69206016 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=33792 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=4,GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=1> grid=1024 block=64 lds=71216 ws=0 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=8772 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=1,GPMPC_DISABLE_GRID_ROOT=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=1,GRID=0> grid=256 block=256 lds=163776 ws=0 zero=0 | nh_max=87 lds_shared=1368 lds_per_wave=4776 linv_in_lds=1 ws_chain_stride=3794 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=4,GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_kernel<T=3,RPL=2,FAC_LDS=0> grid=1024 block=64 lds=15536 ws=57016320 zero=0 | nh_max=87 lds_shared=130 lds_per_wave=1812 linv_in_lds=1 ws_chain_stride=6960 max_points=30'),
    (PEND, R, 3, 1024, 30, 0, 0, 0, 0, 'pin=1,GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_fast_kernel<T=3,NR=36,G_NY=1,ENV=pendulum,LHH_LDS=0,GRID=1> grid=256 block=256 lds=32960 ws=31212544 zero=1 | nh_max=87 lds_shared=0 lds_per_wave=1030 linv_in_lds=1 ws_chain_stride=3810 max_points=30'),
    (CAR, R, 3, 4096, 40, 0, 0, 0, 0, 'GPMPC_FORCE_GLOBAL_FACTOR=1',
     'rollout_tiles_kernel<N0=5,N1=9,ENV=car,NT=32,SEED=0> grid=4096 block=64 lds=40608 ws=1107296256 zero=0 | nh_max=117 lds_shared=252 lds_per_wave=2694 linv_in_lds=1 ws_chain_stride=33792 max_points=40'),
]


def _raw():
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.gpmpc_debug_rollout_plan.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] +
                                             [ctypes.c_int32] * 5 + [ctypes.c_char_p, ctypes.c_size_t])
    return raw


def _descs(desc):
    g_ny, T, N_r, grad, grid = desc
    d = _lib.make_gp_desc(g_ny, 2, T, N_r, grad, [[2.0, 1.1]] * g_ny, [0.05] * g_ny, [2e-7] * T, 1e-20, grid=grid)
    if g_ny == 1:
        e = _lib.make_env_desc(_lib.ENV_PENDULUM1D, 2, 1, False, 0.01, 1.0, 1.0, None, [0, 0])
    else:
        e = _lib.make_env_desc(_lib.ENV_CAR_RESIDUAL, 4, 2, False, 0.06, 1.1, 1.7, None, [0] * 4)
    return d, e


@pytest.mark.parametrize("desc,mode,hall_tasks,Ns,H,n_h0,n_v0,state_slots,state_points,knobs,expected", PLANS)
def test_rollout_plan(monkeypatch, desc, mode, hall_tasks, Ns, H, n_h0, n_v0, state_slots, state_points, knobs, expected):
    raw, lib = _raw(), _lib.load()
    d, e = _descs(desc)
    pin = _lib.KERNEL_AUTO
    for kv in filter(None, knobs.split(",")):
        name, _, val = kv.partition("=")
        if name == "pin":
            pin = int(val)
        else:
            monkeypatch.setenv(name, val)
    prev = lib.gpmpc_rollout_pin_kernel(pin)
    try:
        buf = ctypes.create_string_buffer(512)
        rc = raw.gpmpc_debug_rollout_plan(ctypes.addressof(d), ctypes.addressof(e), mode, hall_tasks, Ns, H, n_h0, n_v0, state_slots,
                                          state_points, buf, 512)
        kernel = lib.gpmpc_rollout_kernel_for(d, e, mode, hall_tasks, Ns, H)
    finally:
        lib.gpmpc_rollout_pin_kernel(prev)
    assert rc == 0
    line = buf.value.decode()
    assert line == expected
    if n_h0 == n_v0 == state_slots == 0 and not line.startswith("error"):
        assert kernel == KERNELS[line.split("<")[0]]
    # what the launch needs fits what the workspace query of the same call returns
    if state_slots == 0 and not line.startswith("error"):
        need = int(re.search(r" ws=(\d+) ", line).group(1))
        if n_h0 == n_v0 == 0:
            assert need <= lib.gpmpc_rollout_workspace_bytes(d, mode, hall_tasks, Ns, H)
        else:
            assert need <= lib.gpmpc_rollout_seeded_workspace_bytes(d, mode, hall_tasks, Ns, H, n_h0, n_v0)


# (descriptor, query, hall_tasks, Ns, n_h0, n_v0): gpmpc_rollout_workspace_bytes ("plain") / gpmpc_rollout_seeded_workspace_bytes in mode R
# for H = 2 .. 65.  Callers allocate by these values: they do not change.
WORKSPACE = {
    ('PEND', 'plain', 3, 1024, 0, 0): [  # unseeded, hall_tasks 3, Ns 1024
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69748736, 73115648, 76556288, 80070656, 83658752, 87320576, 91056128, 94865408,
        98748416, 102705152, 107479296, 110839808, 115017728, 119269376, 123594752, 127993856,
        132466688, 137013248, 141633536, 146327552, 151095296, 155936768, 160851968, 165840896,
        170903552, 176039936, 181250048, 186533888, 191891456, 197322752, 202827776, 208406528,
    ],
    ('PEND', 'plain', 1, 1024, 0, 0): [  # unseeded, hall_tasks 1
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 107479296, 107479296, 107479296, 107479296, 107479296, 107479296,
        107479296, 107479296, 107479296, 107479296, 107479296, 154140928, 154140928, 154140928,
        154140928, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928,
    ],
    ('PEND', 'plain', 3, 4097, 0, 0): [  # unseeded, Ns 4097
        277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656,
        277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656,
        277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656,
        277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656, 277094656,
        279057152, 292527872, 306294016, 320354816, 334710784, 349361664, 364307456, 379548160,
        395084032, 410914816, 430336256, 443461376, 460177152, 477187840, 494493696, 512094464,
        529990144, 548180736, 566666496, 585447168, 604522752, 623893248, 643558912, 663519488,
        683774976, 704325632, 725171200, 746311680, 767747072, 789477632, 811503104, 833823488,
    ],
    ('PEND', 'seeded', 3, 1024, 5, 0): [  # seeded, n_h0 5
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69748736, 73115648, 76556288, 80070656, 83658752,
        87320576, 91056128, 94865408, 98748416, 102705152, 107479296, 110839808, 115017728,
        119269376, 123594752, 127993856, 132466688, 137013248, 141633536, 146327552, 151095296,
        155936768, 160851968, 165840896, 170903552, 176039936, 181250048, 186533888, 191891456,
        197322752, 202827776, 208406528, 214059008, 219785216, 225585152, 231458816, 237406208,
    ],
    ('PEND', 'seeded', 1, 1024, 0, 12): [  # seeded, hall_tasks 1, n_v0 12
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 107479296, 107479296,
        107479296, 107479296, 107479296, 107479296, 107479296, 107479296, 107479296, 107479296,
        107479296, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928,
        154140928, 154140928, 154140928, 154140928, 107479296, 154140928, 154140928, 154140928,
        154140928, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928, 154140928,
    ],
    ('PEND', 'seeded', 3, 1024, 0, 0): [  # seeded query, no seeds
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272, 69206272,
        69748736, 73115648, 76556288, 80070656, 83658752, 87320576, 91056128, 94865408,
        98748416, 102705152, 107479296, 110839808, 115017728, 119269376, 123594752, 127993856,
        132466688, 137013248, 141633536, 146327552, 151095296, 155936768, 160851968, 165840896,
        170903552, 176039936, 181250048, 186533888, 191891456, 197322752, 202827776, 208406528,
    ],
    ('CAR', 'plain', 3, 1024, 0, 0): [  # unseeded, hall_tasks 3, Ns 1024
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 287172608, 299042816, 311134208,
        323446784, 335980544, 429916416, 429916416, 429916416, 429916416, 429916416, 429916416,
        429916416, 444213248, 458737664, 473483264, 488450048, 616562944, 616562944, 616562944,
        616562944, 616562944, 616562944, 616562944, 616562944, 633104384, 650283008, 667682816,
    ],
    ('CAR', 'plain', 1, 1024, 0, 0): [  # unseeded, hall_tasks 1
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 429916416, 429916416, 429916416, 429916416, 429916416, 429916416,
        429916416, 429916416, 429916416, 429916416, 429916416, 616562944, 616562944, 616562944,
        616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944,
    ],
    ('CAR', 'plain', 3, 4097, 0, 0): [  # unseeded, Ns 4097
        1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848,
        1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848,
        1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848,
        1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1107566848,
        1107566848, 1107566848, 1107566848, 1107566848, 1107566848, 1148964864, 1196457216, 1244834560,
        1294096896, 1344244224, 1720084736, 1720084736, 1720084736, 1720084736, 1720084736, 1720084736,
        1720084736, 1777280768, 1835392512, 1894389504, 1954271232, 2466853120, 2466853120, 2466853120,
        2466853120, 2466853120, 2466853120, 2466853120, 2466853120, 2533029888, 2601761024, 2671377152,
    ],
    ('CAR', 'seeded', 3, 1024, 5, 0): [  # seeded, n_h0 5
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        287172608, 299042816, 311134208, 323446784, 335980544, 429916416, 429916416, 429916416,
        429916416, 429916416, 429916416, 429916416, 444213248, 458737664, 473483264, 488450048,
        616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944,
        633104384, 650283008, 667682816, 685303808, 703145984, 721209344, 739493888, 757999616,
    ],
    ('CAR', 'seeded', 1, 1024, 0, 12): [  # seeded, hall_tasks 1, n_v0 12
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 429916416, 429916416,
        429916416, 429916416, 429916416, 429916416, 429916416, 429916416, 429916416, 429916416,
        429916416, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944,
        616562944, 616562944, 616562944, 616562944, 429916416, 616562944, 616562944, 616562944,
        616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944, 616562944,
    ],
    ('CAR', 'seeded', 3, 1024, 0, 0): [  # seeded query, no seeds
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320, 276824320,
        276824320, 276824320, 276824320, 276824320, 276824320, 287172608, 299042816, 311134208,
        323446784, 335980544, 429916416, 429916416, 429916416, 429916416, 429916416, 429916416,
        429916416, 444213248, 458737664, 473483264, 488450048, 616562944, 616562944, 616562944,
        616562944, 616562944, 616562944, 616562944, 616562944, 633104384, 650283008, 667682816,
    ],
}


@pytest.mark.parametrize("key", list(WORKSPACE), ids=lambda k: "-".join(str(v) for v in k))
def test_rollout_workspace_queries(key):
    lib = _lib.load()
    name, query, hall_tasks, Ns, n_h0, n_v0 = key
    d, _ = _descs({"PEND": PEND, "CAR": CAR}[name])
    got = [lib.gpmpc_rollout_workspace_bytes(d, R, hall_tasks, Ns, H) if query == "plain" else
           lib.gpmpc_rollout_seeded_workspace_bytes(d, R, hall_tasks, Ns, H, n_h0, n_v0) for H in range(2, 66)]
    assert got == WORKSPACE[key]
    # mode I keeps no factor
    assert lib.gpmpc_rollout_workspace_bytes(d, I, hall_tasks, Ns, 30) == 256
