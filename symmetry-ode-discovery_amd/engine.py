"""ctypes binding of libsymode_hip.so (C ABI: include/symode.h) on PyTorch-ROCm tensors.

PyTorch is used here for device memory, streams and nothing else: every method takes CUDA
(= HIP) fp32 tensors, hands their ``data_ptr()`` to the C ABI on torch's current stream and
returns tensors allocated by torch.  There is NO CPU fallback: a missing library, a missing
GPU or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes
import functools
import os
import weakref
from ctypes import c_char_p, c_float, c_int, c_long, c_size_t, c_void_p

import torch

FLAG_SINE = 1
FLAG_EXP = 2

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SYMODE_LIB") or os.path.join(_HERE, "libsymode_hip.so")

# name -> (restype, argtypes); kept in step with include/symode.h (tests check every symbol)
_SIGNATURES = {
    "symode_abi_version": (c_int, []),
    "symode_reload_env": (None, []),
    "symode_error_string": (c_char_p, [c_int]),
    "symode_lib_size": (c_int, [c_int, c_int, c_int]),
    "symode_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_long, c_long]),
    "symode_workspace_init": (c_int, [c_void_p, c_size_t, c_void_p]),
    "symode_theta": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p]),
    "symode_forward": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_odeint": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_int,
                              c_void_p, c_void_p]),
    "symode_odeint_traj": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_int,
                              c_void_p, c_void_p]),
    "symode_rollout_error": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_long, c_float, c_int,
                                     c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_loss_grad": (c_int, [c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_float,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_aug_gram": (c_int, [c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "symode_aug_gram_gather": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "symode_symreg_linear": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_symreg_reversed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_symreg_reversed_batched": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int, c_void_p,
                                               c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_weak_gram": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "symode_weak_normal_windows": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_long, c_long, c_void_p, c_void_p,
                                           c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_reversed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_jacobian_constant": (c_int, [c_void_p, c_int, c_long, c_long, c_int, c_void_p, c_void_p, c_void_p]),
    "symode_symreg_reversed_batched_constj": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int,
                                                      c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_reversed_constj": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int,
                                                 c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t,
                                                 c_void_p]),
    "symode_symreg_reversed_batched_constj_live": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int,
                                                           c_void_p, c_void_p, ctypes.c_ulonglong, c_float, c_void_p, c_void_p,
                                                           c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_reversed_constj_live": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int,
                                                      c_int, c_void_p, c_void_p, ctypes.c_ulonglong, c_float, c_float, c_void_p,
                                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_linear_action": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_void_p]),
    "symode_loss_grad_reversed_linear": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int,
                                                 c_int, c_int, c_void_p, c_void_p, ctypes.c_ulonglong, c_float, c_float, c_void_p,
                                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_reversed_linear_gram": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_long,
                                                      c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_ulonglong, c_float, c_float,
                                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_reversed_linear_quad": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_int, c_void_p, c_void_p,
                                                      c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_void_p, ctypes.c_ulonglong, ctypes.c_double,
                                                      c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_size_t, c_void_p]),
    "symode_quad_reduce": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_int, c_int, c_int, ctypes.c_ulonglong,
                                   ctypes.c_double, c_float, c_void_p, c_void_p, c_void_p]),
    "symode_quad_step": (c_int, [c_void_p, c_long, c_int, c_int, c_int, ctypes.c_ulonglong, c_void_p, c_long, c_void_p, c_long,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_loss_grad_latent": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p,
                                        c_float, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_symreg_reversed_gram_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_long, c_long]),
    "symode_symreg_reversed_gram": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_long, c_int, c_int, c_int, c_void_p,
                                            c_void_p, c_size_t, c_void_p]),
    "symode_symreg_reversed_gram_gather_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_long, c_long]),
    "symode_symreg_reversed_gram_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p, c_long, c_long, c_int,
                                                   c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_quad_closure": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, ctypes.c_double, c_float,
                                    c_void_p, c_void_p, c_void_p]),
    "symode_vjp": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_size_t, c_void_p]),
    "symode_forward_jvp": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "symode_jvp_vjp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_rk4_traj": (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_int, ctypes.c_double, c_int, c_void_p, c_void_p,
                                c_void_p]),
    "symode_seeded_subsamples": (c_int, [c_long, c_long, c_void_p, c_int, c_void_p, c_void_p]),
    "symode_euler_jvp": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_void_p,
                                 c_void_p, c_void_p]),
    "symode_euler_jvp_vjp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p,
                                     c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "symode_lbfgs_direction": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                       c_int, c_void_p, c_void_p]),
    "symode_selftest_wave_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "symode_lbfgs_step": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_float, c_float] + [c_void_p] * 15
                          + [c_long, c_int, c_int, c_float, c_float, c_void_p]),
    "symode_trainer_layout": (c_size_t, [c_long, c_int, c_int, c_int, c_int, c_void_p]),
    "symode_trainer_init": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_trainer_closure": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_trainer_update": (c_int, [c_void_p, c_int, c_void_p]),
    "symode_trainer_epoch_end": (c_int, [c_void_p, c_int, c_void_p]),
    "symode_trainer_run": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "symode_trainer_grid_closure": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_trainer_grid_update": (c_int, [c_void_p, c_int, c_void_p]),
    "symode_trainer_grid_epoch_end": (c_int, [c_void_p, c_int, c_void_p]),
    "symode_trainer_grid_run": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "symode_quad_closure_grid": (c_int, [c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_void_p, c_void_p, ctypes.c_double,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_adam_epochs": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_long, c_int, c_int, c_int,
                                   c_void_p, c_int, c_int, c_int] + [c_float] * 6 + [c_int, c_float, c_int, c_int, c_float]
                           + [c_void_p] * 8),
    "symode_adam_epochs_reversed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p, c_long, c_int, c_int,
                                            c_int, c_long, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int] + [c_float] * 7
                                    + [c_int, c_float, c_int, c_int, c_float] + [c_void_p] * 8),
    "symode_adam_epochs_latent": (c_int, [c_void_p] * 5 + [c_int, c_void_p, c_int, c_long, c_void_p, c_long, c_int, c_int, c_int,
                                          c_long, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int] + [c_float] * 8
                                  + [c_int, c_float, c_int, c_int, c_float] + [c_void_p] * 8),
    # the keyed siblings: (idx, n_idx_problems, n_epochs, n_steps, batch) -> (order_seeds, n_order_seeds, shuffle, n_epochs, batch)
    "symode_adam_epochs_keyed": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_long, c_int, c_int,
                                         c_int, c_void_p, c_int, c_int, c_int] + [c_float] * 6
                                 + [c_int, c_float, c_int, c_int, c_float] + [c_void_p] * 8),
    "symode_adam_epochs_reversed_keyed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p, c_long, c_int,
                                                  c_int, c_int, c_long, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int]
                                          + [c_float] * 7 + [c_int, c_float, c_int, c_int, c_float] + [c_void_p] * 8),
    "symode_adam_epochs_latent_keyed": (c_int, [c_void_p] * 5 + [c_int, c_void_p, c_int, c_long, c_void_p, c_long, c_int, c_int,
                                                c_int, c_long, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int]
                                        + [c_float] * 8 + [c_int, c_float, c_int, c_int, c_float] + [c_void_p] * 8),
    "symode_adam_order_table": (c_int, [c_long, c_int, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p]),
    "symode_adam_run": (c_int, [c_void_p, c_void_p]),
    "symode_host_stlsq_sweep": (c_int, [c_void_p, c_int, c_int, c_int, c_long, ctypes.c_double, ctypes.c_double, c_int, c_int,
                                        ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_sweep": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_long, c_void_p, ctypes.c_double, ctypes.c_double, c_int,
                                   ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_sweep_constrained": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_long, c_void_p, c_void_p, c_int, c_int,
                                               c_void_p, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_sweep_minnorm": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_long, c_void_p, c_void_p, c_int, c_int,
                                           c_void_p, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_sweep_symreg": (c_int, [c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_long, c_void_p, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_path": (c_int, [c_void_p, c_void_p, c_long, c_long, c_long, c_int, c_int, c_long, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_path_symreg": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_long, c_long, c_int, c_int, c_long, c_void_p,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_gram_resample": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "symode_stlsq_bag": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                 ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "symode_host_lstsq_normal": (c_int, [c_void_p, c_void_p, c_int, c_int, c_long, c_int, ctypes.c_double, c_void_p, c_void_p]),
}

ABI_VERSION = 8
LBFGS_ACCEPT, LBFGS_BEGIN = 1, 2                            # SYMODE_LBFGS_* of include/symode.h
CLOSURE_STREAM, CLOSURE_GRAM, CLOSURE_LATENT = 0, 1, 2      # SYMODE_CLOSURE_* of include/symode.h


class TrainerDesc(ctypes.Structure):
    """``symode_trainer`` of include/symode.h, field for field."""
    _fields_ = [("x", c_void_p), ("dx", c_void_p), ("gx", c_void_p), ("jgx", c_void_p), ("n_g", c_int), ("w_sym", c_float),
                ("n_problems", c_long), ("n_points", c_long), ("d", c_int), ("order", c_int), ("flags", c_int),
                ("inv_count", c_float), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("q_eff", c_void_p), ("r", c_int), ("allow_constant", c_int), ("n_params", c_int),
                ("w_x", c_float), ("w_reg", c_float), ("l1", c_int), ("lr", c_float), ("tol_grad", c_float), ("tol_change", c_float),
                ("max_iter", c_int), ("history", c_int),
                ("threshold", c_float), ("tol_update", c_float), ("near_band", c_float), ("st_freq", c_int),
                ("state", c_void_p), ("state_bytes", c_size_t),
                ("log", c_void_p), ("log_test", c_void_p), ("log_xi", c_void_p), ("log_mask", c_void_p), ("log_params", c_void_p), ("log_epochs", c_int),
                ("aug_gram", c_void_p), ("rev_gram", c_void_p),
                ("closure", c_int), ("latent_B", c_void_p), ("latent_y", c_void_p)]


TRAINER_HYPER = 4                                           # SYMODE_TRAINER_HYPER: columns of a row, lr, w_reg, threshold, w_sym


class TrainerGrid(ctypes.Structure):
    """``symode_trainer_grid`` of include/symode.h, field for field."""
    _fields_ = [("base", TrainerDesc), ("hyper", c_void_p), ("n_sets", c_long)]


STLSQ_HYPER = 2                                             # columns of a symode_stlsq_sweep hyper row: gamma, threshold
STLSQ_SYMREG_HYPER = 3                                      # ... of a symode_stlsq_sweep_symreg row: gamma, threshold, w_sym
STLSQ_PATH_SYMREG_HYPER = 2                                 # ... of a symode_stlsq_path_symreg row: gamma, w_sym

_PACKED = {"f8": (8, torch.float64, "<f8"), "f4": (4, torch.float32, "<f4"), "i4": (4, torch.int32, "<i4"), "u1": (1, torch.uint8, "u1")}


def packed_layout(fields, S, n_tail=None):
    """Where the small outputs of one STLSQ launch lie in the ONE uint8 buffer they share, so that a caller on the host fetches
    all of them in one copy.  ``fields``: (name, "f8" | "f4" | "i4" | "u1", per-problem shape) in the order the caller wants them
    back; each holds S problems.  The parts are placed by descending item size -- fp64, then fp32 and int32, bytes last -- so
    every part starts at a multiple of its own item size; ``n_tail`` int32 (None: no tail) ride 4-aligned behind the last byte
    field.  A plain function of sizes.  Returns (bytes, views): ``views(buf)`` gives {name: typed (S, *shape) view} in the
    fields' order, "tail" last, of a torch uint8 tensor or of the numpy uint8 array one copy of it made."""
    spans, at = {}, 0
    for name, kind, shape in sorted(fields, key=lambda f: -_PACKED[f[1]][0]):
        n = _PACKED[kind][0] * S
        for extent in shape:
            n *= extent
        spans[name] = (at, at + n)
        at += n
    at = -(-at // 4) * 4                                                # the tail, int32-aligned behind the last byte field
    end = at + 4 * (n_tail or 0)
    # per part: its span, its type (None: the buffer's own bytes) and its shape (None: the flat (S,) the span already is)
    plan = [(name,) + spans[name] + (None if kind == "u1" else _PACKED[kind], (S,) + tuple(shape) if shape else None)
            for name, kind, shape in fields]
    if n_tail is not None:
        plan.append(("tail", at, end, _PACKED["i4"], None))

    def views(buf):
        which = 1 if isinstance(buf, torch.Tensor) else 2
        out = {}
        for name, lo, hi, kind, shape in plan:
            part = buf[lo:hi] if kind is None else buf[lo:hi].view(kind[which])
            out[name] = part if shape is None else part.reshape(shape)
        return out

    return end, views


def stlsq_fields(entry, d, p, r1=0):
    """The small outputs of the launch ``entry`` as ``packed_layout`` takes them, in the order its wrapper returns them; ``r1`` =
    r' of the constrained fits, n0 = d p the joint support of the regularised path."""
    n0 = d * p
    sweep = [("xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("passes", "i4", ()), ("near", "i4", ()), ("fell", "i4", ())]
    return {
        "symode_stlsq_sweep": sweep,
        "symode_stlsq_sweep_symreg": sweep,
        "symode_stlsq_sweep_constrained": sweep + [("var", "f4", (r1,))],
        "symode_stlsq_sweep_minnorm": sweep + [("var", "f4", (r1,)), ("trunc", "i4", ()), ("rank", "i4", ())],
        "symode_stlsq_path": [("Xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("order", "i4", (d, p)), ("rss_train", "f8", (d, p + 1)),
                              ("rss_val", "f8", (d, p + 1)), ("best", "i4", (d,)), ("near", "i4", ()), ("fell", "i4", ())],
        "symode_stlsq_path_symreg": [("Xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("order", "i4", (n0,)), ("mse_train", "f8", (n0 + 1,)),
                                     ("reg_train", "f8", (n0 + 1,)), ("mse_val", "f8", (n0 + 1,)), ("best", "i4", ()),
                                     ("near", "i4", ()), ("fell", "i4", ())],
        # (count, valid, mean and std are per seed: the launch writes the first n_seeds rows of theirs)
        "symode_stlsq_bag": [("xi", "f4", (d, p)), ("mask", "u1", (d, p)), ("fell", "i4", ()), ("count", "i4", (d, p)),
                             ("valid", "i4", ()), ("mean", "f8", (d, p)), ("std", "f8", (d, p))],
    }[entry]


@functools.lru_cache(maxsize=4096)
def _stlsq_layout(entry, S, d, p, r1, n_tail):
    """``packed_layout`` of a launch's ``stlsq_fields``: a function of six sizes, worked out once per shape"""
    return packed_layout(stlsq_fields(entry, d, p, r1), S, n_tail)

ADAM_PLAIN, ADAM_REVERSED, ADAM_LATENT = 0, 1, 2              # SYMODE_ADAM_* of include/symode.h
ADAM_HYPER = 4                                              # columns of a hyper row: lr, w_reg, threshold, w_sym


class AdamJob(ctypes.Structure):
    """``symode_adam_job`` of include/symode.h, field for field."""
    _fields_ = [("kind", c_int), ("x", c_void_p), ("dx", c_void_p), ("n_src", c_long),
                ("gx", c_void_p), ("jgx", c_void_p), ("n_g", c_int), ("D_obs", c_int),
                ("lat_B", c_void_p), ("lat_y", c_void_p), ("lat_e", c_void_p), ("lat_L", c_void_p), ("n_gen", c_int),
                ("n_steps", c_int), ("idx", c_void_p), ("n_idx_problems", c_long),
                ("order_seeds", c_void_p), ("n_order_seeds", c_long), ("shuffle", c_int),
                ("n_epochs", c_int), ("batch", c_int), ("n_problems", c_long), ("d", c_int), ("order", c_int), ("flags", c_int),
                ("q_eff", c_void_p), ("r", c_int), ("allow_constant", c_int), ("n_params", c_int),
                ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("w_x", c_float), ("w_obs", c_float),
                ("w_reg", c_float), ("w_sym", c_float), ("l1", c_int), ("threshold", c_float), ("st_freq", c_int), ("epoch0", c_int),
                ("near_band", c_float),
                ("params", c_void_p), ("m", c_void_p), ("v", c_void_p), ("step", c_void_p), ("mask", c_void_p), ("xi_out", c_void_p),
                ("log", c_void_p), ("hyper", c_void_p)]


TRAINER_FIELDS = ("params", "xi", "mask", "cl_loss", "cl_grad", "g", "loss", "act", "n_iter", "d", "t", "old_dirs", "old_stps", "ro",
                  "head", "count", "h_diag", "prev_g", "prev_loss", "prev", "pprev", "n_iters", "done", "nan", "finished", "epochs",
                  "near", "l1_last", "test_grad")


class SymodeError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """dlopen the HIP library and declare every entry point; raises if it is not built."""
    if not os.path.exists(path):
        raise SymodeError(
            f"{path} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    if lib.symode_abi_version() != ABI_VERSION:
        raise SymodeError(f"libsymode_hip ABI {lib.symode_abi_version()} != binding ABI {ABI_VERSION}")
    return lib


def reload_env() -> None:
    """Have the loaded library read its optional SYMODE_* variables again (it reads them once, at first use)."""
    if _ENGINE is not None:
        _ENGINE.lib.symode_reload_env()


def library_flags(include_sine: bool, include_exp: bool) -> int:
    return (FLAG_SINE if include_sine else 0) | (FLAG_EXP if include_exp else 0)


# The native entry of the step on the reduced form (csrc/step_entry.cpp -> _symode_step*.so beside the library).  Optional at
# import: without it ``quad_step_plan`` hands out the Python ``ReducedStep``, and these two say so.
try:
    from . import _symode_step as _step_entry
    step_entry_loaded, step_entry_error = True, None
except ImportError as _e:
    _step_entry, step_entry_loaded, step_entry_error = None, False, f"{type(_e).__name__}: {_e}"

# what a prepared step answers in the place of its result tuple (None: the library's switches refuse the step)
STEP_STALE, STEP_SLOW = -1001, -1002                      # STALE / SLOW of csrc/step_entry.cpp, clear of the SYMODE_E_* codes


def step_entry_enabled() -> bool:
    """Does ``quad_step_plan`` hand out the native plan?  The module loaded and SYMODE_STEP_ENTRY is not 0; read where a plan is
    made, not per call."""
    return step_entry_loaded and os.environ.get("SYMODE_STEP_ENTRY", "1")[:1] != "0"


def step_key(x, dx, sym, Q, live):
    """What a reduced form was built from: (version, pointer) of x, dx, gx, jgx and Q, the weight and the column set; ``sym`` =
    (gx, jgx, weight).  The native plan reads the same twelve components from the same five arguments."""
    gx, jgx, weight = sym
    return (x._version, x.data_ptr(), dx._version, dx.data_ptr(), gx._version, gx.data_ptr(), jgx._version, jgx.data_ptr(),
            weight, live, Q._version, Q.data_ptr())


class ReducedStep:
    """A prepared ``symode_quad_step`` launch on one reduced form B (``HipEngine.quad_step_plan``): the pointers, sizes and
    header arguments that stand while B stands are kept, so that a call is one allocation -- a packed fp32 buffer
    [loss (S) | g_beta (S, r) | g_const (S, d_c)] of which the results are views -- and one ctypes call.  ``alias=True``
    writes into one buffer of this object instead and returns the same views every time.
    This is the step in Python: what ``quad_step_plan`` hands out where the native plan (csrc/step_entry.cpp, which does the
    same in one call) is not built or SYMODE_STEP_ENTRY=0, and where the native plan sends operands it does not take."""

    def __init__(self, eng, B, order, live, r, dc, ws, key=None):
        self.eng, self.B, self.ws = eng, B, ws                       # kept alive with the pointers below
        self.key = None if key is None else step_key(*key)
        self.S, self.r, self.dc, self.device = B.shape[0], r, dc, B.device
        self._fn = eng.lib.symode_quad_step
        self._head = (B.data_ptr(), self.S, r + dc, dc, order, live)
        self._tail = (ws.data_ptr(), ws.numel() * 8)
        self._sizes = [self.S, self.S * r, self.S * dc] if dc else [self.S, self.S * r]
        self._n_out = sum(self._sizes)
        self._alias = None

    def _views(self, buf):
        parts = buf.split_with_sizes(self._sizes)
        return parts[0], parts[1].view(self.S, self.r), (parts[2].view(self.S, self.dc, 1) if self.dc else None)

    def _rows(self, t, w, name):
        """(tensor, row stride) of an (S, w[, 1]) fp32 operand read where it lies; anything else is made dense first"""
        S = self.S
        st = t.stride()
        if t.dtype is torch.float32 and t.device == self.device and len(st) >= 2 and t.shape[0] == S and t.shape[1] == w \
                and t.numel() == S * w and st[1] == 1 and (st[0] >= w or S == 1):
            return t, (st[0] if S > 1 else w)
        t = HipEngine._dev(t, name)
        if t.numel() != S * w:
            raise SymodeError(f"{name} has {t.numel()} elements, expected {S}x{w}")
        return t, w

    def __call__(self, args):
        """``args`` = (anything, beta, const, alias[, x, dx, sym, Q, live]), the tuple of ``loss_grad_reversed(reduced=)``.
        (loss, g_beta, g_const or None); None where the library's switches refuse the step (SYMODE_QUAD_REDUCED=0 and the
        switches of the closure it stands for): the caller then takes that closure's own launch; STEP_STALE where the five
        key operands are given and ``step_key`` of them is not the key this step was made with."""
        if len(args) > 4 and step_key(*args[4:]) != self.key:
            return STEP_STALE
        return self.step(args[1], args[2], args[3])

    def step(self, beta, const, alias=False):
        beta, ldb = self._rows(beta, self.r, "beta")
        if self.dc:
            const, ldc = self._rows(const, self.dc, "const")
            cptr = const.data_ptr()
        else:
            cptr, ldc = None, 0
        if alias:
            if self._alias is None:
                buf = torch.empty(self._n_out, dtype=torch.float32, device=self.device)
                self._alias = (buf, self._views(buf))
            buf, views = self._alias
        else:
            buf, views = torch.empty(self._n_out, dtype=torch.float32, device=self.device), None
        base = buf.data_ptr()
        S4 = 4 * self.S
        rc = self._fn(*self._head, beta.data_ptr(), ldb, cptr, ldc, base, base + S4, (base + S4 * (1 + self.r)) if self.dc else None,
                      *self._tail, torch.cuda.current_stream(self.device).cuda_stream)
        if rc == -1:                                                 # SYMODE_E_UNSUPPORTED: a switch, read by the library alone
            return None
        if rc != 0:
            self.eng._check(rc, "symode_quad_step")
        return self._views(buf) if views is None else views


class HipEngine:
    """The product's only compute backend for the hot path."""

    def __init__(self, path: str = LIB_PATH):
        self.lib = load_library(path)
        self._ws = {}     # (device index, stream) -> scratch tensor (grown on demand, reused)
        # did the native step entry load, and if not why (the module's own record, also on the instance)
        self.step_entry_loaded, self.step_entry_error = step_entry_loaded, step_entry_error

    # -- plumbing ----------------------------------------------------------------------
    def _check(self, code: int, what: str):
        if code > 0:
            # a HIP error from a launch: whatever state the scratch buffers' tickets are in, the next call gets fresh ones
            self._ws.clear()
        if code != 0:
            raise SymodeError(f"{what} failed: {self.lib.symode_error_string(code).decode()} (code {code})")

    @staticmethod
    def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SymodeError(f"{name} must be a CUDA/HIP tensor; the hot path has no CPU fallback")
        if t.dtype != dtype:
            raise SymodeError(f"{name} must be {dtype}, got {t.dtype}")
        return t.contiguous()

    @staticmethod
    def _dev_or_pinned(t: torch.Tensor, name: str) -> torch.Tensor:
        """fp32 device tensor, or a pinned host tensor (hipHostMalloc memory is mapped into the device's address space
        at the same address): lets a latency-bound caller hand coefficients in and take [loss | grad] out of ONE launch
        without copy nodes on either side."""
        if isinstance(t, torch.Tensor) and not t.is_cuda and t.is_pinned() and t.dtype == torch.float32 and t.is_contiguous():
            return t
        return HipEngine._dev(t, name)

    @staticmethod
    def _ptr(t):
        return None if t is None else c_void_p(t.data_ptr())

    @staticmethod
    def _stream(t: torch.Tensor):
        return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    # -- the operands of the symode_stlsq_* launches, each rule stated once (the tensors have been through _dev) --
    @staticmethod
    def _stlsq_G(G, d):
        """(n_sets, p) of the augmented Gram matrices"""
        if G.dim() != 3 or G.shape[1] != G.shape[2] or G.shape[1] <= d:
            raise SymodeError(f"G must be (n_sets, p + d, p + d) with d = {d}, got {tuple(G.shape)}")
        return G.shape[0], G.shape[1] - d

    @staticmethod
    def _stlsq_V(V, G):
        if V.dim() != 3 or V.shape[1:] != G.shape[1:] or V.device != G.device:
            raise SymodeError(f"V must be (n_val_sets, p + d, p + d) = (n_val_sets, {G.shape[1]}, {G.shape[2]}) on {G.device}, "
                              f"got {tuple(V.shape)} on {V.device}")

    @staticmethod
    def _stlsq_R(R, G, n_sets, n0):
        if tuple(R.shape) != (n_sets, n0, n0) or R.device != G.device:
            raise SymodeError(f"R must be (n_sets, d p, d p) = ({n_sets}, {n0}, {n0}) fp64 on {G.device}, got {tuple(R.shape)}")

    def _stlsq_Q(self, q_solve, q_xi, allow_constant, G, d, p):
        """(q_solve, q_xi, r, r') of the constrained fits"""
        q_solve, q_xi = self._dev(q_solve, "q_solve", torch.float64), self._dev(q_xi, "q_xi")
        if q_xi.dim() != 2 or q_xi.shape[0] != d * p or q_xi.device != G.device:
            raise SymodeError(f"q_xi must be (d p, r) = ({d * p}, r) fp32 on {G.device}, got {tuple(q_xi.shape)}")
        r = q_xi.shape[1]
        R = r + (d if allow_constant else 0)
        if tuple(q_solve.shape) != (d * p, R) or q_solve.device != G.device:
            raise SymodeError(f"q_solve must be (d p, r') = ({d * p}, {R}) fp64 on {G.device}, got {tuple(q_solve.shape)}")
        return q_solve, q_xi, r, R

    def _stlsq_hyper(self, hyper, n_problems, G, columns, row):
        """(hyper, S): the per-problem table of ``columns`` values (``row`` names them) and the number of problems, which
        defaults to the table's rows, or to G's sets without a table"""
        if hyper is not None:
            hyper = self._dev(hyper, "hyper")
            if hyper.dim() != 2 or hyper.shape[1] != columns or hyper.device != G.device:
                raise SymodeError(f"hyper must be (n_problems, {columns}) fp32 on {G.device}: one row [{row}] per problem")
            if n_problems is not None and int(n_problems) != hyper.shape[0]:
                raise SymodeError(f"hyper has {hyper.shape[0]} rows for {n_problems} problems")
            n_problems = hyper.shape[0]
        return hyper, G.shape[0] if n_problems is None else int(n_problems)

    def _stlsq_outputs(self, G, entry, S, d, p, r1=0, tail=None):
        """The outputs of the launch ``entry`` in one allocation (``packed_layout``), the tail copied in: ({name: device view},
        fetch) with ``fetch(to_host)`` -> the same views, or numpy views of ONE copy of the buffer."""
        n_bytes, views = _stlsq_layout(entry, S, d, p, r1, None if tail is None else tail.numel())
        buf = torch.empty(max(n_bytes, 0), dtype=torch.uint8, device=G.device)
        out = views(buf)
        if tail is not None:
            out["tail"].copy_(self._dev(tail, "tail", torch.int32).reshape(-1))
        return out, lambda to_host: views(buf.cpu().numpy()) if to_host else out

    def lib_size(self, d: int, order: int, flags: int) -> int:
        p = self.lib.symode_lib_size(d, order, flags)
        if p < 0:
            raise SymodeError(f"library d={d} order={order} flags={flags} is not compiled into libsymode_hip")
        return p

    def workspace(self, device, d, order, flags, n_problems, n, min_bytes=0) -> torch.Tensor:
        need = max(self.lib.symode_workspace_bytes(d, order, flags, n_problems, n), min_bytes)
        dev = torch.device(device)
        key = (dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)   # one scratch per (device, stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() * 8 < need:
            ws = self.new_workspace(dev, need)
            self._ws[key] = ws
        return ws

    def new_workspace(self, device, nbytes) -> torch.Tensor:
        """A private scratch buffer, header initialised on the current stream (symode_workspace_init): for callers
        that replay launches from a HIP graph or from several streams in turn and must not share the engine's."""
        ws = torch.empty(max(nbytes // 8 + 1, 1024), dtype=torch.float64, device=device)
        self._check(self.lib.symode_workspace_init(self._ptr(ws), ws.numel() * 8, self._stream(ws)), "symode_workspace_init")
        return ws

    # -- entry points ------------------------------------------------------------------
    def theta(self, x, order, flags=0):
        x = self._dev(x, "x")
        lead, d = x.shape[:-1], x.shape[-1]
        n = x.numel() // d if d else 0
        p = self.lib_size(d, order, flags)
        out = torch.empty(*lead, p, dtype=torch.float32, device=x.device)
        self._check(self.lib.symode_theta(self._ptr(x), n, d, order, flags, self._ptr(out), self._stream(x)), "symode_theta")
        return out

    def forward(self, x, xi, mask, order, flags=0):
        x = self._dev(x, "x")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, _ = self._coef(xi, mask, d, order, flags)
        out = torch.empty_like(x)
        self._check(self.lib.symode_forward(self._ptr(x), n, d, order, flags, self._ptr(xi), self._ptr(mask),
                                            self._ptr(out), self._stream(x)), "symode_forward")
        return out

    def odeint(self, x, xi, mask, order, flags, n_steps, dt, method="euler"):
        x = self._dev(x, "x")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, _ = self._coef(xi, mask, d, order, flags)
        m = self._method_code(method)
        out = torch.empty_like(x)
        self._check(self.lib.symode_odeint(self._ptr(x), n, d, order, flags, self._ptr(xi), self._ptr(mask), int(n_steps),
                                           float(dt), m, self._ptr(out), self._stream(x)), "symode_odeint")
        return out

    def odeint_traj(self, x, xi, mask, order, flags, n_steps, dt, method="euler"):
        """(n_steps, n, d): the state after every step (odeint(..., full_traj=True))."""
        x = self._dev(x, "x")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, _ = self._coef(xi, mask, d, order, flags)
        m = self._method_code(method)
        traj = torch.empty(int(n_steps), n, d, dtype=torch.float32, device=x.device)
        self._check(self.lib.symode_odeint_traj(self._ptr(x), n, d, order, flags, self._ptr(xi), self._ptr(mask), int(n_steps),
                                                float(dt), m, self._ptr(traj), self._stream(x)), "symode_odeint_traj")
        return traj

    def rollout_error(self, x_true, xi, mask, order, flags, dt, method="rk4", bound=float("inf"), want_error=True):
        """Roll-out error of S models on held-out trajectories in ONE launch (symode_rollout_error).  x_true (n_ics,
        n_steps + 1, d): the integration starts at x_true[:, 0]; xi, mask (S, d, p) or (d, p), mask may be None.
        Returns (err (S, n_ics, n_steps) fp32 -- None with ``want_error=False`` --, mean_err (S, n_ics) fp64, horizon
        (S, n_ics) int32: leading steps with err <= bound; bound = inf counts the leading finite steps)."""
        x_true = self._dev(x_true, "x_true")
        if x_true.dim() != 3:
            raise SymodeError(f"x_true must be (n_ics, n_steps + 1, d), got {tuple(x_true.shape)}")
        n_ics, n_points, d = x_true.shape
        S = xi.shape[0] if isinstance(xi, torch.Tensor) and xi.dim() == 3 else 1
        xi, mask, _ = self._coef(xi, mask, d, order, flags, S)
        m = self._method_code(method)
        n_steps = n_points - 1
        err = torch.empty(S, n_ics, max(n_steps, 0), dtype=torch.float32, device=x_true.device) if want_error else None
        mean_err = torch.empty(S, n_ics, dtype=torch.float64, device=x_true.device)
        horizon = torch.empty(S, n_ics, dtype=torch.int32, device=x_true.device)
        self._check(self.lib.symode_rollout_error(self._ptr(x_true), n_ics, n_steps, d, order, flags, self._ptr(xi),
                                                  self._ptr(mask), S, float(dt), m, float(bound), self._ptr(err),
                                                  self._ptr(mean_err), self._ptr(horizon), self._stream(x_true)),
                    "symode_rollout_error")
        return err, mean_err, horizon

    def adam_epochs(self, x, dx, idx, params, m, v, step, mask, order, flags=0, *, lr, betas=(0.9, 0.999), eps=1e-8, w_x=1.0,
                    w_reg=0.0, l1=True, threshold=0.0, st_freq=0, epoch0=0, near_band=1e-4, q_eff=None, allow_constant=True,
                    hyper=None, _reversed=None, _latent=None, _keyed=None):
        """``idx.shape[0]`` whole epochs of minibatch Adam steps for S problems in ONE launch (symode_adam_epochs).
        x, dx (n_src, d) fp32; idx (n_epochs, S or 1, n_steps, batch) int32 row numbers; params, m, v (S, n_params) fp32,
        step (S,) int32 and mask (S, d, p) fp32 are the state, UPDATED IN PLACE (so they must be contiguous); q_eff
        (d p, r) fp32 or None (the parameters are Xi).  ``idx`` is NOT range-checked here: the kernel treats every entry
        outside [0, n_src) as padding -- not read, not counted in the batch's divisor (-1 is the canonical pad).
        Returns (xi (S, d, p), log (n_epochs, S, 8)); log columns: mean batch MSE, mean |params|_1, steps taken,
        near-threshold coefficients at the epoch's event, frozen-after-NaN flag, thresholding event, epoch, 0.
        ``hyper``: None, or a contiguous (S, 4) fp32 tensor on the device of x whose row s is problem s's own
        [lr, w_reg, threshold, w_sym] (symode_adam_run): the launch then reads none of the scalars ``lr``, ``w_reg``,
        ``threshold``, ``w_sym``, and problem s is bit for bit the scalar launch on problem s alone with row s's values.  The
        reversed, latent and keyed wrappers hand it through."""
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        if x.dim() != 2 or dx.shape != x.shape:
            raise SymodeError(f"x and dx must both be (n_src, d), got {tuple(x.shape)} and {tuple(dx.shape)}")
        n_src, d = x.shape
        p = self.lib_size(d, order, flags)
        seeds = None
        if _keyed is not None:                               # the *_keyed entries: no table, see adam_epochs_keyed
            if idx is not None:
                raise SymodeError("a keyed launch takes order seeds in place of idx, not both")
            seeds, n_epochs, batch, shuffle = _keyed
            seeds, n_epochs, batch = self._order_seeds(seeds, x.device), int(n_epochs), int(batch)
            if n_epochs < 0 or batch < 1:
                raise SymodeError(f"a keyed launch needs n_epochs >= 0 and batch >= 1, got {n_epochs} and {batch}")
        elif not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 4 or not idx.is_contiguous():
            raise SymodeError("idx must be a contiguous (n_epochs, S or 1, n_steps, batch) int32 CUDA/HIP tensor")
        for name, t in (("dx", dx), ("idx", idx), ("order_seeds", seeds), ("params", params), ("m", m), ("v", v), ("step", step), ("mask", mask), ("q_eff", q_eff)):
            if isinstance(t, torch.Tensor) and t.device != x.device:
                raise SymodeError(f"{name} is on {t.device}, x on {x.device}: all tensors of one launch live on one device")
        state = {"params": params, "m": m, "v": v, "mask": mask}
        for name, t in state.items():
            if self._dev(t, name) is not t:
                raise SymodeError(f"{name} is updated in place and must be contiguous")
        if self._dev(step, "step", torch.int32) is not step:
            raise SymodeError("step is updated in place and must be contiguous")
        if params.dim() != 2 or m.shape != params.shape or v.shape != params.shape:
            raise SymodeError(f"params, m, v must share one (S, n_params) shape, got {tuple(params.shape)}, {tuple(m.shape)}, {tuple(v.shape)}")
        S, n_params = params.shape
        if step.shape != (S,):
            raise SymodeError(f"step must be ({S},), got {tuple(step.shape)}")
        if mask.numel() != S * d * p:
            raise SymodeError(f"mask has {mask.numel()} elements, expected {S}x{d}x{p}")
        if seeds is None:
            n_epochs, n_tab, n_steps, batch = idx.shape
            if n_tab not in (1, S):
                raise SymodeError(f"idx holds {n_tab} tables, expected 1 or {S}")
            suffix, table = "", (self._ptr(idx), n_tab, n_epochs, n_steps, batch)
        else:
            if seeds.numel() not in (1, S):
                raise SymodeError(f"order_seeds holds {seeds.numel()} seeds, expected 1 or {S}")
            suffix, table = "_keyed", (self._ptr(seeds), seeds.numel(), int(bool(shuffle)), n_epochs, batch)
        r = 0
        if q_eff is not None:
            q_eff = self._dev(q_eff, "q_eff")
            if q_eff.dim() != 2 or q_eff.shape[0] != d * p:
                raise SymodeError(f"q_eff must be ({d * p}, r), got {tuple(q_eff.shape)}")
            r = q_eff.shape[1]
        if n_params != (r + d if q_eff is not None else d * p):
            raise SymodeError(f"params has {n_params} columns, expected {r + d if q_eff is not None else d * p}")
        xi = torch.empty(S, d, p, dtype=torch.float32, device=x.device)
        log = torch.empty(n_epochs, S, 10 if _latent is not None else 8, dtype=torch.float32, device=x.device)
        if hyper is not None:
            if (not isinstance(hyper, torch.Tensor) or not hyper.is_cuda or hyper.dtype != torch.float32
                    or tuple(hyper.shape) != (S, ADAM_HYPER) or not hyper.is_contiguous() or hyper.device != x.device):
                raise SymodeError(f"hyper must be a contiguous ({S}, {ADAM_HYPER}) fp32 tensor on {x.device}: one row "
                                  "[lr, w_reg, threshold, w_sym] per problem")
            J = AdamJob(kind=ADAM_PLAIN, x=x.data_ptr(), dx=dx.data_ptr(), n_src=n_src, n_epochs=n_epochs, batch=batch, n_problems=S,
                        d=d, order=order, flags=flags, q_eff=None if q_eff is None else q_eff.data_ptr(), r=r,
                        allow_constant=int(bool(allow_constant)), n_params=n_params, lr=float(lr), beta1=float(betas[0]),
                        beta2=float(betas[1]), eps=float(eps), w_x=float(w_x), w_reg=float(w_reg), l1=int(bool(l1)),
                        threshold=float(threshold), st_freq=int(st_freq), epoch0=int(epoch0), near_band=float(near_band),
                        params=params.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), step=step.data_ptr(), mask=mask.data_ptr(),
                        xi_out=xi.data_ptr(), log=log.data_ptr(), hyper=hyper.data_ptr())
            if seeds is None:
                J.idx, J.n_idx_problems, J.n_steps = idx.data_ptr(), n_tab, n_steps
            else:
                J.order_seeds, J.n_order_seeds, J.shuffle = seeds.data_ptr(), seeds.numel(), int(bool(shuffle))
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            if _latent is not None:
                B, y, e, D_obs, L, n_gen, w_z, w_sym = _latent
                J.kind, J.lat_B, J.lat_y, J.lat_e, J.lat_L, J.D_obs, J.n_gen = ADAM_LATENT, ptr(B), ptr(y), ptr(e), ptr(L), D_obs, n_gen
                J.w_x, J.w_obs, J.w_sym = float(w_z), float(w_x), float(w_sym)
            elif _reversed is not None:
                gx, jgx, n_g, w_sym = _reversed
                J.kind, J.gx, J.jgx, J.n_g, J.w_sym = ADAM_REVERSED, ptr(gx), ptr(jgx), n_g, float(w_sym)
            self._check(self.lib.symode_adam_run(ctypes.byref(J), self._stream(x)), "symode_adam_run")
            return xi, log
        if _latent is not None:
            B, y, e, D_obs, L, n_gen, w_z, w_sym = _latent
            self._check(getattr(self.lib, "symode_adam_epochs_latent" + suffix)(
                self._ptr(x), self._ptr(dx), self._ptr(B), self._ptr(y), self._ptr(e), D_obs, self._ptr(L), n_gen, n_src,
                *table, S, d, order, flags, self._ptr(q_eff), r,
                int(bool(allow_constant)), n_params, float(lr), float(betas[0]), float(betas[1]), float(eps), float(w_z),
                float(w_x), float(w_reg), float(w_sym), int(bool(l1)), float(threshold), int(st_freq), int(epoch0),
                float(near_band), self._ptr(params), self._ptr(m), self._ptr(v), self._ptr(step), self._ptr(mask),
                self._ptr(xi), self._ptr(log), self._stream(x)), "symode_adam_epochs_latent" + suffix)
            return xi, log
        if _reversed is not None:
            gx, jgx, n_g, w_sym = _reversed
            self._check(getattr(self.lib, "symode_adam_epochs_reversed" + suffix)(
                self._ptr(x), self._ptr(dx), self._ptr(gx), self._ptr(jgx), n_g, n_src, *table, S, d, order, flags, self._ptr(q_eff), r, int(bool(allow_constant)), n_params, float(lr), float(betas[0]),
                float(betas[1]), float(eps), float(w_x), float(w_reg), float(w_sym), int(bool(l1)), float(threshold),
                int(st_freq), int(epoch0), float(near_band), self._ptr(params), self._ptr(m), self._ptr(v), self._ptr(step),
                self._ptr(mask), self._ptr(xi), self._ptr(log), self._stream(x)), "symode_adam_epochs_reversed" + suffix)
            return xi, log
        self._check(getattr(self.lib, "symode_adam_epochs" + suffix)(
            self._ptr(x), self._ptr(dx), n_src, *table, S, d, order, flags,
            self._ptr(q_eff), r, int(bool(allow_constant)), n_params, float(lr), float(betas[0]), float(betas[1]), float(eps),
            float(w_x), float(w_reg), int(bool(l1)), float(threshold), int(st_freq), int(epoch0), float(near_band),
            self._ptr(params), self._ptr(m), self._ptr(v), self._ptr(step), self._ptr(mask), self._ptr(xi), self._ptr(log),
            self._stream(x)), "symode_adam_epochs" + suffix)
        return xi, log

    def _order_seeds(self, seeds, device):
        """Order seeds as the keyed entries read them: a contiguous int64 device tensor (a sequence of Python integers of any
        size is taken modulo 2^64, as the subsample seeds are)."""
        if isinstance(seeds, torch.Tensor):
            if not seeds.is_cuda or seeds.dtype != torch.int64 or seeds.dim() != 1 or not seeds.is_contiguous():
                raise SymodeError("order_seeds must be a contiguous 1-D int64 CUDA/HIP tensor or a sequence of integers")
            return seeds
        words = [((int(s) & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)) - (1 << 63) for s in seeds]
        return torch.tensor(words, dtype=torch.int64, device=device)

    def adam_epochs_keyed(self, x, dx, order_seeds, n_epochs, batch, params, m, v, step, mask, order, flags=0, *, shuffle=True,
                          **kw):
        """``adam_epochs`` without an index table (symode_adam_epochs_keyed): batch slot b of step s in epoch e reads the row
        at position s * batch + b of the order ``device_adam.epoch_order(order seed, epoch0 + e, n_src)``, computed inside
        the launch (``shuffle=False``: the row is the position).  ``order_seeds``: one integer (every problem walks the
        same order) or S of them, a sequence or an int64 device tensor.  The other arguments and the return value are those
        of ``adam_epochs``; the state it leaves is, bit for bit, that of ``adam_epochs`` on ``adam_order_table``."""
        return self.adam_epochs(x, dx, None, params, m, v, step, mask, order, flags,
                                _keyed=(order_seeds, n_epochs, batch, shuffle), **kw)

    def adam_epochs_reversed_keyed(self, x, dx, gx, jgx, order_seeds, n_epochs, batch, params, m, v, step, mask, order, flags=0,
                                   *, shuffle=True, **kw):
        """``adam_epochs_reversed`` on the computed order of ``adam_epochs_keyed`` (symode_adam_epochs_reversed_keyed)."""
        return self.adam_epochs_reversed(x, dx, gx, jgx, None, params, m, v, step, mask, order, flags,
                                         _keyed=(order_seeds, n_epochs, batch, shuffle), **kw)

    def adam_epochs_latent_keyed(self, z, dz, B, y, e, D_obs, L, order_seeds, n_epochs, batch, params, m, v, step, mask, order,
                                 flags=0, *, shuffle=True, **kw):
        """``adam_epochs_latent`` on the computed order of ``adam_epochs_keyed`` (symode_adam_epochs_latent_keyed)."""
        return self.adam_epochs_latent(z, dz, B, y, e, D_obs, L, None, params, m, v, step, mask, order, flags,
                                       _keyed=(order_seeds, n_epochs, batch, shuffle), **kw)

    def adam_order_table(self, n_src, batch, order_seeds, n_epochs, epoch0=0, shuffle=True, device=None):
        """The (n_epochs, len(order_seeds), ceil(n_src / batch), batch) int32 table the keyed launches walk, written by the
        device function they use (symode_adam_order_table): rows of epochs epoch0 .. epoch0 + n_epochs - 1, -1 beyond
        n_src.  ``device``: where a sequence of seeds goes (default: the current device)."""
        seeds = self._order_seeds(order_seeds, torch.device('cuda', torch.cuda.current_device()) if device is None else device)
        n_src, batch, n_epochs = int(n_src), int(batch), int(n_epochs)
        if n_src < 1 or batch < 1 or n_epochs < 0 or seeds.numel() < 1:
            raise SymodeError(f"adam_order_table needs n_src >= 1, batch >= 1, n_epochs >= 0 and a seed, got {n_src}, {batch}, "
                              f"{n_epochs}, {seeds.numel()}")
        idx = torch.empty(n_epochs, seeds.numel(), (n_src + batch - 1) // batch, batch, dtype=torch.int32, device=seeds.device)
        with torch.cuda.device(seeds.device):
            self._check(self.lib.symode_adam_order_table(n_src, batch, self._ptr(seeds), seeds.numel(), int(bool(shuffle)),
                                                         int(epoch0), n_epochs, self._ptr(idx), self._stream(seeds)),
                        "symode_adam_order_table")
        return idx

    def adam_epochs_reversed(self, x, dx, gx, jgx, idx, params, m, v, step, mask, order, flags=0, *, w_sym, **kw):
        """``adam_epochs`` with the reversed symmetry regulariser in every minibatch loss (symode_adam_epochs_reversed):
        ``w_x * mse + w_sym * sum_g mean |J_g(x) h(x) - h(g x)|^2 + w_reg * |params|_1`` on gx (n_g, n_src, d) and jgx
        (n_g, n_src, d, d) fp32, computed once for the data set and gathered by the same row numbers as x and dx (padding
        reads none of them).  n_g = 0 (gx, jgx may be None) is ``adam_epochs`` bit for bit.  The other arguments and the
        return value are those of ``adam_epochs``; log column 7 is the epoch mean of the batch regulariser (unweighted).
        n_g > 0 needs w_x > 0."""
        x = self._dev(x, "x")
        if x.dim() != 2:
            raise SymodeError(f"x must be (n_src, d), got {tuple(x.shape)}")
        n_src, d = x.shape
        n_g = 0
        if gx is not None or jgx is not None:
            if gx is None or jgx is None:
                raise SymodeError("gx and jgx are given together or not at all")
            gx, jgx = self._dev(gx, "gx"), self._dev(jgx, "jgx")
            if gx.dim() != 3 or gx.shape[1:] != (n_src, d) or jgx.shape != (gx.shape[0], n_src, d, d):
                raise SymodeError(f"gx must be (n_g, {n_src}, {d}) and jgx (n_g, {n_src}, {d}, {d}), got {tuple(gx.shape)} and "
                                  f"{tuple(jgx.shape)}")
            if gx.device != x.device or jgx.device != x.device:
                raise SymodeError(f"gx / jgx are on {gx.device} / {jgx.device}, x on {x.device}: all tensors of one launch "
                                  "live on one device")
            n_g = gx.shape[0]
        if n_g == 0:
            gx = jgx = None
        return self.adam_epochs(x, dx, idx, params, m, v, step, mask, order, flags, _reversed=(gx, jgx, n_g, w_sym), **kw)

    def adam_epochs_latent(self, z, dz, B, y, e, D_obs, L, idx, params, m, v, step, mask, order, flags=0, *, w_z, w_sym, **kw):
        """``adam_epochs`` on the latent branch (symode_adam_epochs_latent): per minibatch
        ``w_z * mse_z + w_x * mse_x + w_sym * sum_g sum_b |W J_Theta(z)(L_g z) - L_g W Theta(z)|^2 + w_reg * |params|_1`` on the
        per-row operands of ``model_utils.latent_operands``: z, dz, y (n_src, d), B (n_src, d, d), e (n_src,) or None when
        D_obs == d, and the generators L (n_gen, d, d) or None (n_gen = 0), all fp32.  mse_x is logged and added but has no
        gradient; the regulariser is not divided by the rows.  The other arguments are those of ``adam_epochs``; returns
        (xi (S, d, p), log (n_epochs, S, 10)): columns 0-6 as ``adam_epochs`` with 0 = mean mse_x, 7 = mean regulariser,
        8 = mean mse_z, 9 = 0.  Needs w_z > 0."""
        z = self._dev(z, "z")
        if z.dim() != 2:
            raise SymodeError(f"z must be (n_src, d), got {tuple(z.shape)}")
        n_src, d = z.shape
        B, y = self._dev(B, "B"), self._dev(y, "y")
        if B.shape != (n_src, d, d) or y.shape != (n_src, d):
            raise SymodeError(f"B must be ({n_src}, {d}, {d}) and y ({n_src}, {d}), got {tuple(B.shape)} and {tuple(y.shape)}")
        D_obs = int(D_obs)
        if D_obs < d:
            raise SymodeError(f"D_obs is {D_obs}, below the latent dimension {d}")
        if e is None and D_obs > d:
            raise SymodeError(f"e (n_src,) is needed with D_obs {D_obs} > d {d}")
        if e is not None:
            e = self._dev(e, "e")
            if e.shape != (n_src,):
                raise SymodeError(f"e must be ({n_src},), got {tuple(e.shape)}")
        n_gen = 0
        if L is not None:
            L = self._dev(L, "L")
            if L.dim() != 3 or L.shape[1:] != (d, d):
                raise SymodeError(f"L must be (n_gen, {d}, {d}), got {tuple(L.shape)}")
            n_gen = L.shape[0]
        if n_gen == 0:
            L = None
        for name, t in (("B", B), ("y", y), ("e", e), ("L", L)):
            if t is not None and t.device != z.device:
                raise SymodeError(f"{name} is on {t.device}, z on {z.device}: all tensors of one launch live on one device")
        return self.adam_epochs(z, dz, idx, params, m, v, step, mask, order, flags, _latent=(B, y, e, D_obs, L, n_gen, w_z, w_sym), **kw)

    def _check_coef(self, xi, mask, d, order, flags, n_problems=1):
        p = self.lib_size(d, order, flags)
        want = n_problems * d * p
        if xi.numel() != want:
            raise SymodeError(f"xi has {xi.numel()} elements, expected {n_problems}x{d}x{p}")
        if mask is not None and mask.numel() != want:
            raise SymodeError(f"mask has {mask.numel()} elements, expected {n_problems}x{d}x{p}")
        return p

    def _coef(self, xi, mask, d, order, flags, n_problems=1, pinned_ok=False):
        """The coefficient operands of every entry point: (xi, mask or None, p), fp32 and contiguous, sizes checked
        against the library.  ``pinned_ok``: xi may be a pinned host tensor (the closures' zero-copy form)."""
        xi = self._dev_or_pinned(xi, "xi") if pinned_ok else self._dev(xi, "xi")
        mask = None if mask is None else self._dev(mask, "mask")
        return xi, mask, self._check_coef(xi, mask, d, order, flags, n_problems)

    @staticmethod
    def _method_code(method):
        m = {"euler": 0, "rk4": 1}.get(method)
        if m is None:
            raise ValueError("Unrecognized ODEInt method.")
        return m

    # -- the closures: loss_grad, symreg_reversed, loss_grad_reversed and bind_closure share everything below ----------
    @staticmethod
    def _problems(x):
        """(batched, S, n, d) of x (S, N, d) or (N, d)."""
        batched = x.dim() == 3
        return batched, x.shape[0] if batched else 1, x.shape[-2], x.shape[-1]

    def _reversed_operands(self, x, gx, jgx, min_n_g=1, compact_ok=False):
        """(g(x), J_g(x)) checked against x: (gx, jgx, n_g, constj).  ``constj``: jgx is the compact table of a
        point-constant Jacobian, (S, n_g, d, d) [one problem: (n_g, d, d)] -- the number of dimensions decides (the
        materialised form has one more, the point axis); recognised only with ``compact_ok``."""
        gx, jgx = self._dev(gx, "gx"), self._dev(jgx, "jgx")
        batched, S, n, d = self._problems(x)
        n_g = gx.shape[1] if batched else gx.shape[0]
        want_g = (S, n_g, n, d) if batched else (n_g, n, d)
        constj = compact_ok and n_g >= 1 and tuple(jgx.shape) == want_g[:-2] + (d, d)
        if n_g < min_n_g or tuple(gx.shape) != want_g or (not constj and tuple(jgx.shape) != want_g + (d,)):
            raise SymodeError(f"gx {tuple(gx.shape)} / jgx {tuple(jgx.shape)} do not match x {tuple(x.shape)}")
        return gx, jgx, n_g, constj

    def _closure_prologue(self, x, S, n, d, p, order, flags, n_loss, out, ws, inv_count):
        """Outputs (allocated, or the caller's ``out`` checked), scratch (the engine's, or a private ``ws`` checked) and
        the 1/count factor of a closure call: (loss, grad, ws, inv)."""
        if out is None:
            loss = torch.empty((S, n_loss) if n_loss > 1 else S, dtype=torch.float32, device=x.device)
            grad = torch.empty(S, d, p, dtype=torch.float32, device=x.device)
        else:
            loss, grad = (self._dev_or_pinned(o, "out") for o in out)
            if loss.numel() != n_loss * S or grad.numel() != S * d * p:
                raise SymodeError(f"out buffers hold {loss.numel()} / {grad.numel()} elements, expected {n_loss * S} / {S * d * p}")
        if ws is None:
            ws = self.workspace(x.device, d, order, flags, S, n)
        elif ws.numel() * 8 < self.lib.symode_workspace_bytes(d, order, flags, S, n):
            raise SymodeError("private workspace too small for this call")
        return loss, grad, ws, 1.0 / (n * d) if inv_count is None else float(inv_count)

    def _closure_call(self, x, dx, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, stream, live=None, linear_m=None,
                      gram=None):
        """One closure launch, ready to go: (entry name, its argument tuple, the tensors the arguments point into, what
        the caller gets back).  ``dx`` None: the regulariser alone; ``rev`` None: the MSE alone, else what
        _reversed_operands returned; ``live``: the set of library columns that may hold a coefficient (an int, bit k =
        column k), honoured by the compact-table forms (their _live entries) and without effect elsewhere.
        ``linear_m``: the substitution matrices of a linear action (``linear_action``), fused compact-table form only: the call
        goes to symode_loss_grad_reversed_linear; ``gram``: with ``linear_m``, the float64 (S, 1, p, p) raw library Gram sums
        of x: the call goes to symode_loss_grad_reversed_linear_gram.  The ONE
        statement of the closures' C signatures: the eager methods call ``getattr(lib, name)(*args)``, bind_closure
        converts ``args`` once and keeps the call."""
        batched, S, n, d = self._problems(x)
        xi, mask, p = self._coef(xi, mask, d, order, flags, S, pinned_ok=True)
        fused = dx is not None and rev is not None
        loss, grad, ws, inv = self._closure_prologue(x, S, n, d, p, order, flags, 2 if fused else 1, out, ws, inv_count)
        head = (self._ptr(x),) if dx is None else (self._ptr(x), self._ptr(dx))
        keep = (x, dx, xi, mask, loss, grad, ws)
        name = "symode_loss_grad"
        live_arg = ()
        if rev is not None:
            gx, jgx, n_g, constj = rev
            head += (self._ptr(gx), self._ptr(jgx), n_g)
            keep += (gx, jgx)
            name = ("symode_loss_grad_reversed" if fused else "symode_symreg_reversed_batched") + ("_constj" if constj else "")
            if linear_m is not None:
                if not (fused and constj and linear_m.dtype == torch.float64 and linear_m.is_contiguous()
                        and linear_m.numel() == S * n_g * p * p):
                    raise SymodeError("linear_m goes with the fused compact-table closure and holds (S, n_g, p, p) float64")
                head = head[:3] + (self._ptr(jgx), self._ptr(linear_m), n_g)
                keep += (linear_m,)
                name, live_arg = "symode_loss_grad_reversed_linear", ((0xFFFFFFFFFFFFFFFF if live is None else int(live)) & 0xFFFFFFFFFFFFFFFF,)
                if gram is not None:
                    if not (gram.is_cuda and gram.dtype == torch.float64 and gram.is_contiguous() and gram.numel() == S * n_g * p * p):
                        raise SymodeError("gram holds (S, 1, p, p) float64 on the device, contiguous")
                    head = head[:5] + (self._ptr(gram),) + head[5:]
                    keep += (gram,)
                    name += "_gram"
            elif gram is not None:
                raise SymodeError("gram goes with linear_m")
            elif constj and live is not None:
                name, live_arg = name + "_live", (int(live) & 0xFFFFFFFFFFFFFFFF,)
        args = head + (S, n, d, order, flags, self._ptr(xi), self._ptr(mask)) + live_arg + (inv,) + ((float(w_sym),) if fused else ()) \
            + (self._ptr(loss), self._ptr(grad), self._ptr(ws), ws.numel() * 8, stream)
        # the outputs in the caller's form: the batch axis is there only if x had one
        loss, grad = loss.reshape(S, 2) if fused else loss.reshape(S), grad.reshape(S, d, p)
        return name, args, keep, (loss, grad) if batched else (loss[0], grad[0])

    def _closure(self, x, dx, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, live=None, linear_m=None, gram=None):
        name, args, _, result = self._closure_call(x, dx, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, self._stream(x),
                                                   live, linear_m, gram)
        self._check(getattr(self.lib, name)(*args), name)
        return result

    def loss_grad(self, x, dx, xi, mask, order, flags=0, inv_count=None, out=None, ws=None):
        """x, dx: (S, N, d) or (N, d); xi, mask: (S, d, p) or (d, p).  Returns (loss (S,), grad (S, d, p)).
        ``xi`` and ``out`` may be pinned host tensors (zero-copy); ``ws`` a private workspace from new_workspace()."""
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        if x.shape != dx.shape:
            raise SymodeError(f"x {tuple(x.shape)} and dx {tuple(dx.shape)} differ")
        return self._closure(x, dx, None, xi, mask, order, flags, None, inv_count, out, ws)

    def aug_gram(self, x, dx, order, flags=0):
        """fp64 augmented Gram [Theta | dx]^T [Theta | dx]: (S, p+d, p+d) or (p+d, p+d)."""
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        if x.shape != dx.shape:
            raise SymodeError(f"x {tuple(x.shape)} and dx {tuple(dx.shape)} differ")
        batched = x.dim() == 3
        S = x.shape[0] if batched else 1
        n, d = x.shape[-2], x.shape[-1]
        p = self.lib_size(d, order, flags)
        gram = torch.empty(S, p + d, p + d, dtype=torch.float64, device=x.device)
        ws = self.workspace(x.device, d, order, flags, S, n)
        self._check(self.lib.symode_aug_gram(self._ptr(x), self._ptr(dx), S, n, d, order, flags, self._ptr(gram),
                                             self._ptr(ws), ws.numel() * 8, self._stream(x)), "symode_aug_gram")
        return gram if batched else gram[0]

    def aug_gram_gather(self, x, dx, idx, order, flags=0):
        """Gram matrices of S index subsets of one shared data set: x, dx (N, d); idx (S, M) int32 rows."""
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        idx = self._dev(idx, "idx", torch.int32)
        if x.dim() != 2 or x.shape != dx.shape or idx.dim() != 2:
            raise SymodeError("aug_gram_gather expects x, dx (N, d) and idx (S, M)")
        n_src, d = x.shape
        S, m = idx.shape
        # the kernel trusts the table: checked once per live table tensor (one reduction, one sync -- ~40 us at config[3]'s
        # 64 x 50 000 rows, more than the 25 us kernel), remembered by object, in-place version and N
        seen = getattr(self, "_idx_checked", None)
        if seen is None or seen[0]() is not idx or seen[1:] != (idx._version, n_src):
            lo, hi = torch.stack(torch.aminmax(idx)).tolist() if idx.numel() else (0, 0)
            if lo < 0 or hi >= max(n_src, 1):
                raise SymodeError("idx holds row indices outside [0, N)")
            self._idx_checked = (weakref.ref(idx), idx._version, n_src)
        p = self.lib_size(d, order, flags)
        gram = torch.empty(S, p + d, p + d, dtype=torch.float64, device=x.device)
        ws = self.workspace(x.device, d, order, flags, S, m)
        self._check(self.lib.symode_aug_gram_gather(self._ptr(x), self._ptr(dx), n_src, self._ptr(idx), S, m, d, order, flags,
                                                    self._ptr(gram), self._ptr(ws), ws.numel() * 8, self._stream(x)),
                    "symode_aug_gram_gather")
        return gram

    def symreg_linear(self, z, xi, mask, L, order, flags=0):
        z = self._dev(z, "z")
        n, d = z.shape[-2], z.shape[-1]
        xi, mask, p = self._coef(xi, mask, d, order, flags)
        L = self._dev(L, "L").reshape(-1, d, d)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        grad = torch.empty(d, p, dtype=torch.float32, device=z.device)
        ws = self.workspace(z.device, d, order, flags, 1, n)
        self._check(self.lib.symode_symreg_linear(self._ptr(z), n, d, order, flags, self._ptr(xi), self._ptr(mask),
                                                  self._ptr(L), L.shape[0], self._ptr(loss), self._ptr(grad),
                                                  self._ptr(ws), ws.numel() * 8, self._stream(z)), "symode_symreg_linear")
        return loss[0], grad

    def symreg_reversed(self, x, gx, jgx, xi, mask, order, flags=0, out=None, ws=None, inv_count=None, live_columns=None):
        """Reversed symmetry regulariser on precomputed (g(x), J_g(x)).
        One problem: x (N, d), gx (n_g, N, d), jgx (n_g, N, d, d), xi / mask (d, p) -> (loss scalar, grad (d, p)).
        S problems in one launch: x (S, N, d), gx (S, n_g, N, d), jgx (S, n_g, N, d, d), xi / mask (S, d, p) -> ((S,), (S, d, p)).
        ``xi`` / ``out`` may be pinned host tensors for the one-problem form; ``inv_count`` as in loss_grad.
        A point-constant Jacobian may be given as its compact table, jgx (n_g, d, d) / (S, n_g, d, d) (``jacobian_constant``):
        the shape alone selects the kernel form that streams nothing of J_g; the results are bit-identical.
        ``live_columns`` as in loss_grad_reversed."""
        x = self._dev(x, "x")
        rev = self._reversed_operands(x, gx, jgx, min_n_g=0, compact_ok=True)
        return self._closure(x, None, rev, xi, mask, order, flags, None, inv_count, out, ws, live_columns)

    def jacobian_constant(self, jgx):
        """Is J_g the same matrix at every point of each (problem, group element)?  jgx (S, n_g, N, d, d) or (n_g, N, d, d)
        -> (table (S, n_g, d, d) or (n_g, d, d), is_constant).  One streaming pass (bitwise comparison with point 0 of every
        slab: -0.0 != +0.0, a NaN answers False) and ONE synchronisation to read the flag: meant to run once per data set.
        With is_constant, ``table`` may be passed as ``jgx`` to symreg_reversed / loss_grad_reversed."""
        jgx = self._dev(jgx, "jgx")
        if jgx.dim() not in (4, 5) or jgx.shape[-1] != jgx.shape[-2] or jgx.numel() == 0:
            raise SymodeError(f"jacobian_constant expects jgx (S, n_g, N, d, d) or (n_g, N, d, d), got {tuple(jgx.shape)}")
        batched = jgx.dim() == 5
        S = jgx.shape[0] if batched else 1
        n_g, n, d = jgx.shape[-4], jgx.shape[-3], jgx.shape[-1]
        table = torch.empty((S, n_g, d, d) if batched else (n_g, d, d), dtype=torch.float32, device=jgx.device)
        flag = torch.empty(1, dtype=torch.int32, device=jgx.device)
        self._check(self.lib.symode_jacobian_constant(self._ptr(jgx), n_g, S, n, d, self._ptr(table), self._ptr(flag),
                                                      self._stream(jgx)), "symode_jacobian_constant")
        return table, bool(flag.item())

    def linear_action(self, x, gx, table, order, flags=0):
        """Is g(x) = J x under the compact table of ``jacobian_constant``?  x (S, N, d), gx (S, 1, N, d), table (S, 1, d, d)
        [one problem: (N, d), (1, N, d), (1, d, d)] -> (M (S, 1, p, p) float64 with Theta(J x) = M Theta(x), is_linear).
        Per component |gx - J x| <= 4 * 2^-24 * |J| |x| in fp64 (symode.h: symode_linear_action); a NaN, an infinity or an
        offset answers False.  d = 2 plain polynomial libraries, one group element.  One streaming pass and ONE
        synchronisation: meant to run once per data set.  With is_linear, ``M`` may be passed as ``linear_m`` to
        loss_grad_reversed."""
        x, gx, table = self._dev(x, "x"), self._dev(gx, "gx"), self._dev(table, "table")
        batched, S, n, d = self._problems(x)
        n_g = gx.shape[-3]
        if tuple(gx.shape) != ((S, n_g, n, d) if batched else (n_g, n, d)) or tuple(table.shape) != tuple(gx.shape[:-2]) + (d, d):
            raise SymodeError(f"gx {tuple(gx.shape)} / table {tuple(table.shape)} do not match x {tuple(x.shape)}")
        p = self.lib_size(d, order, flags)
        m = torch.empty((S, n_g, p, p) if batched else (n_g, p, p), dtype=torch.float64, device=x.device)
        flag = torch.empty(1, dtype=torch.int32, device=x.device)
        self._check(self.lib.symode_linear_action(self._ptr(x), self._ptr(gx), self._ptr(table), n_g, S, n, d, order, flags,
                                                  self._ptr(m), self._ptr(flag), self._stream(x)), "symode_linear_action")
        return m, bool(flag.item())

    @staticmethod
    def closure_body(ws):
        """Which body the last reversed-closure launch on workspace ``ws`` took: "scalar", "packed" (the packed-fp32 body of the
        compact-table form, d = 2; SYMODE_CLOSURE_PK=0 turns it off), either with "-live" where it was the kernel that leaves out
        the columns outside ``live_columns`` (SYMODE_CLOSURE_LIVE=0 turns that off), "fold" / "fold-live" for the kernel of a linear
        action that reads no g(x) (``linear_m``; SYMODE_CLOSURE_FOLD=0 turns it off), or None before any.  The kernel leaves it in word 1 of the
        workspace header (an initialised workspace only, and only its LAST launch is visible): the two bodies return the same
        bits, so the results cannot tell.  One synchronisation."""
        return {1: "scalar", 2: "packed", 5: "scalar-live", 6: "packed-live", 8: "fold", 12: "fold-live"}.get(int(ws.view(torch.int64)[1].item()) & 15)

    @staticmethod
    def closure_levers(ws):
        """(packed body, chunk addressing in SGPRs) of the last fold launch on workspace ``ws`` (closure_fold.hpp; SYMODE_FOLD_PK=0
        turns both off): bits 16 and 32 of the word ``closure_body`` reads.  Both are bit-identical to the plain fold kernel."""
        word = int(ws.view(torch.int64)[1].item())
        return bool(word & 16), bool(word & 32)

    @staticmethod
    def closure_gram(ws):
        """Did the last fold launch on workspace ``ws`` take the Gram form (closure_fold.hpp: the regulariser from the library
        Gram, once per problem; SYMODE_FOLD_GRAM=0 turns it off)?  Bit 64 of the word ``closure_body`` reads."""
        return bool(int(ws.view(torch.int64)[1].item()) & 64)

    @staticmethod
    def closure_quad(ws):
        """Did the last fold launch on workspace ``ws`` run without a point loop (closure_quad.hpp: residual and regulariser from
        the augmented Gram, ``aug=``; SYMODE_FOLD_RESID_GRAM=0 turns it off)?  Bit 128 of the word ``closure_body`` reads."""
        return bool(int(ws.view(torch.int64)[1].item()) & 128)

    @staticmethod
    def closure_quad_enabled():
        """Do the library's switches allow the ``aug=`` route (symode_loss_grad_reversed_linear_quad)?  The three variables as
        the library reads them (off when the value starts with '0' / is the number 0); the library reads them at load and at
        ``reload_env``, and refuses the call where they say no -- a caller that wants the point-loop kernels then asks here."""
        env = os.environ
        return not (env.get("SYMODE_CLOSURE_FOLD", "1")[:1] == "0" or env.get("SYMODE_FOLD_RESID_GRAM", "1")[:1] == "0"
                    or env.get("SYMODE_FOLD_GRAM", "1").strip() in ("0", "+0", "-0", "00", ""))

    @staticmethod
    def closure_reduced(ws):
        """Was the last closure launch on workspace ``ws`` the step on the reduced form (closure_reduced.hpp: ``quad_step``, a
        quadratic form in (beta, const); SYMODE_QUAD_REDUCED=0 turns it off)?  Bit 256 of the word ``closure_body`` reads."""
        return bool(int(ws.view(torch.int64)[1].item()) & 256)

    @staticmethod
    def closure_reduced_enabled():
        """Do the library's switches allow ``quad_reduce`` / ``quad_step``?  Those of ``closure_quad_enabled`` and
        SYMODE_QUAD_REDUCED, as the library reads them; it refuses the calls where they say no."""
        return HipEngine.closure_quad_enabled() and os.environ.get("SYMODE_QUAD_REDUCED", "1")[:1] != "0"

    def quad_reduce(self, aug, linear_m, table, order, coef, w_sym, inv_count, live_columns=None, mask=None):
        """The closure of ``loss_grad_reversed(aug=, coef=)`` reduced to a quadratic form in the variables (symode_quad_reduce):
        aug (S, p+d, p+d) float64, linear_m (S, 1, p, p) float64, table (S, 1, d, d) fp32, ``coef`` a CoefMap with Q, mask
        (S, d, p) fp32 or None -> B (S, K+1, K+1) float64, K = r + (d if the model reads const else 0), with
        loss = v^T B v and d loss / d (beta, const) = 2 (B v)[:K] for v = [beta; const; 1].  A set-up call: B holds for these
        operands, ``w_sym``, ``inv_count`` and ``live_columns`` and is built again when any of them changes."""
        aug, linear_m, table = self._dev(aug, "aug", torch.float64), self._dev(linear_m, "linear_m", torch.float64), self._dev(table, "table")
        d, p, r = coef.d, coef.p, coef.r
        if d != 2 or coef.Q is None or r < 1:
            raise SymodeError("quad_reduce takes a d = 2 coefficient map with Q")
        if aug.dim() != 3 or aug.shape[1:] != (p + d, p + d):
            raise SymodeError(f"aug holds (S, p+d, p+d) float64, got {tuple(aug.shape)}")
        S = aug.shape[0]
        if linear_m.numel() != S * p * p or table.numel() != S * d * d:
            raise SymodeError(f"linear_m {tuple(linear_m.shape)} / table {tuple(table.shape)} do not hold (S, 1, p, p) / (S, 1, d, d)")
        mask = None if mask is None else self._dev(mask, "mask")
        if mask is not None and mask.numel() != S * d * p:
            raise SymodeError(f"mask has {mask.numel()} elements, expected {S}x{d}x{p}")
        K = r + (d if coef.allow_constant else 0)
        if K + 1 > 16:
            raise SymodeError(f"the reduced form holds at most 15 variables per problem, the map has {K}")
        Q = coef.device_Q(aug.device)
        live = (0xFFFFFFFFFFFFFFFF if live_columns is None else int(live_columns)) & 0xFFFFFFFFFFFFFFFF
        B = torch.empty(S, K + 1, K + 1, dtype=torch.float64, device=aug.device)
        self._check(self.lib.symode_quad_reduce(self._ptr(aug), self._ptr(linear_m), self._ptr(table), S, order, self._ptr(Q), r,
                                                1 if coef.use_kron else 0, 1 if coef.allow_constant else 0, live, float(inv_count),
                                                float(w_sym), self._ptr(mask), self._ptr(B), self._stream(aug)), "symode_quad_reduce")
        return B

    def quad_step(self, B, beta, const, order, live_columns=None, out=None, ws=None):
        """One closure evaluation on the reduced form (symode_quad_step): B (S, K+1, K+1) float64 of ``quad_reduce``, beta
        (S, r) fp32, const (S, d_c, 1) fp32 or None (K = r + d_c); rows of beta and const may be strided (views of a flat
        [beta | const] state), only the last axis has to be dense.  Returns (loss (S,), g_beta (S, r), g_const (S, d_c, 1) or
        None), fp32; ``out`` = (loss, g_beta, g_const or None): buffers for them.  ``order`` and ``live_columns`` name the
        closure B was reduced from: the launch leaves that closure's header word, plus bit 256, in ``ws``."""
        B = self._dev(B, "B", torch.float64)
        if B.dim() != 3 or B.shape[1] != B.shape[2] or not 2 <= B.shape[1] <= 16:
            raise SymodeError(f"B holds (S, K+1, K+1) float64 with K + 1 <= 16, got {tuple(B.shape)}")
        S, K = B.shape[0], B.shape[1] - 1
        rows = lambda t, w: t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.shape[0] == S and t.numel() == S * w \
            and all(st == 1 for st in t.stride()[1:]) and t.stride(0) >= w
        dc = 0 if const is None else const.numel() // S
        r = K - dc
        if r < 1 or (const is not None and const.numel() != S * dc):
            raise SymodeError(f"const has {0 if const is None else const.numel()} elements for {S} problems of {K} variables")
        beta = beta if rows(beta, r) else self._dev(beta, "beta")
        if beta.numel() != S * r:
            raise SymodeError(f"beta has {beta.numel()} elements, expected {S}x{r}")
        if const is not None and not rows(const, dc):
            const = self._dev(const, "const")
        ld = lambda t, w: t.stride(0) if (t.dim() >= 2 and t.shape[0] == S and S > 1) else w
        dev = B.device
        if out is None:
            loss = torch.empty(S, dtype=torch.float32, device=dev)
            g_beta = torch.empty(S, r, dtype=torch.float32, device=dev)
            g_const = torch.empty(S, dc, 1, dtype=torch.float32, device=dev) if dc else None
        else:
            loss, g_beta, g_const = (None if o is None else self._dev(o, "out") for o in out)
            if loss is None or g_beta is None or loss.numel() != S or g_beta.numel() != S * r or (g_const is None) != (dc == 0) \
                    or (g_const is not None and g_const.numel() != S * dc):
                raise SymodeError("out = (loss (S,), g_beta (S, r), g_const (S, d_c, 1) or None)")
        if ws is None:
            ws = self.workspace(dev, 2, order, 0, S, 1)
        live = (0xFFFFFFFFFFFFFFFF if live_columns is None else int(live_columns)) & 0xFFFFFFFFFFFFFFFF
        self._check(self.lib.symode_quad_step(self._ptr(B), S, K, dc, order, live, self._ptr(beta), ld(beta, r), self._ptr(const),
                                              0 if const is None else ld(const, dc), self._ptr(loss), self._ptr(g_beta),
                                              self._ptr(g_const), self._ptr(ws), ws.numel() * 8, self._stream(B)), "symode_quad_step")
        return loss, g_beta.reshape(S, r), None if g_const is None else g_const.reshape(S, dc, 1)

    def quad_step_plan(self, B, order, live_columns, r, dc, ws, key=None):
        """The step on B, prepared: everything of ``quad_step`` that cannot change while B stands.  ``key`` = (x, dx, sym, Q,
        live), the operands B was reduced from as a call will name them (``step_key``): a call that names operands of another
        key answers STEP_STALE.  With a key, where ``step_entry_enabled()``, the result is the native plan
        (``_symode_step.Plan``: key, row checks, allocation, stream, launch and views in one call; its ``slow`` is the
        ``ReducedStep`` for operands it does not take); else the ``ReducedStep`` itself.  Both are called with the tuple of
        ``loss_grad_reversed(reduced=)``."""
        B = self._dev(B, "B", torch.float64)
        K = r + dc
        if B.dim() != 3 or tuple(B.shape[1:]) != (K + 1, K + 1) or r < 1 or dc < 0 or K + 1 > 16:
            raise SymodeError(f"B {tuple(B.shape)} does not hold (S, K+1, K+1) for K = {r} + {dc} <= 15")
        if ws is None or not ws.is_cuda or ws.dtype != torch.float64 or ws.device != B.device:
            raise SymodeError("the prepared step takes an initialised workspace on B's device (new_workspace)")
        live = (0xFFFFFFFFFFFFFFFF if live_columns is None else int(live_columns)) & 0xFFFFFFFFFFFFFFFF
        slow = ReducedStep(self, B, order, live, r, dc, ws, key)
        if key is None or not step_entry_enabled():
            return slow
        address = ctypes.cast(self.lib.symode_quad_step, c_void_p).value
        return _step_entry.Plan(address, B, ws, r, dc, order, live, key, slow)

    def _closure_quad_call(self, x, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, live, linear_m, aug, coef, coef_out):
        """The launch of ``loss_grad_reversed(aug=...)``: the arguments of symode_loss_grad_reversed_linear_quad, checked."""
        batched, S, n, d = self._problems(x)
        gx, jgx, n_g, constj = rev
        p = self.lib_size(d, order, flags)
        if not (constj and linear_m is not None and linear_m.is_cuda and linear_m.dtype == torch.float64 and linear_m.is_contiguous()
                and linear_m.numel() == S * n_g * p * p):
            raise SymodeError("aug goes with the compact table and linear_m, (S, n_g, p, p) float64 on the device, contiguous")
        if not (aug.is_cuda and aug.dtype == torch.float64 and aug.is_contiguous() and aug.numel() == S * (p + d) * (p + d)):
            raise SymodeError("aug holds (S, p+d, p+d) float64 on the device, contiguous")
        mask = None if mask is None else self._dev(mask, "mask")
        if mask is not None and mask.numel() != S * d * p:
            raise SymodeError(f"mask has {mask.numel()} elements, expected {S}x{d}x{p}")
        dev = x.device
        keep = [aug, linear_m, jgx, mask]
        if coef is None:
            xi = self._dev(xi, "xi")
            if xi.numel() != S * d * p:
                raise SymodeError(f"xi has {xi.numel()} elements, expected {S}x{d}x{p}")
            map_args, extra = (self._ptr(xi), None, None, 0, None, 0, 0, 0), (None, None, None)
            keep.append(xi)
            mapped = ()
        else:
            cmap, beta, const = coef
            Q = cmap.device_Q(dev)
            r = cmap.r
            # rows of a flat [beta | const] state are taken where they lie: only the last axis has to be dense
            rows = lambda t, w: t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.shape[0] == S and t.numel() == S * w \
                and all(st == 1 for st in t.stride()[1:]) and t.stride(0) >= w
            beta = beta if rows(beta, r) else self._dev(beta, "beta")
            if (cmap.d, cmap.p) != (d, p) or beta.numel() != S * r:
                raise SymodeError(f"coef maps ({cmap.d}, {cmap.p}) from {r} variables; beta has {beta.numel()} elements for {S} problems of ({d}, {p})")
            const = None if (const is None or not cmap.allow_constant) else (const if rows(const, d) else self._dev(const, "const"))
            if const is not None and const.numel() != S * d:
                raise SymodeError(f"const has {const.numel()} elements, expected {S}x{d}")
            if coef_out is None:
                xi_out = None
                g_beta = torch.empty(S, r, dtype=torch.float32, device=dev)
                g_const = torch.empty(S, d, 1, dtype=torch.float32, device=dev) if cmap.allow_constant else None
            else:
                xi_out, g_beta, g_const = (None if o is None else self._dev(o, "coef_out") for o in coef_out)
                if g_beta is None or g_beta.numel() != S * r or (g_const is not None and g_const.numel() != S * d) or \
                        (xi_out is not None and xi_out.numel() != S * d * p):
                    raise SymodeError("coef_out = (xi_out (S, d, p) or None, g_beta (S, r), g_const (S, d, 1) or None)")
            ld = lambda t, w: t.stride(0) if (t.dim() >= 2 and t.shape[0] == S and S > 1) else w
            map_args = (None, self._ptr(Q), self._ptr(beta), ld(beta, r), self._ptr(const), 0 if const is None else ld(const, d), r,
                        1 if cmap.use_kron else 0)
            extra = (self._ptr(xi_out), self._ptr(g_beta), self._ptr(g_const))
            keep += [Q, beta, const, xi_out, g_beta, g_const]
            mapped = (g_beta.reshape(S, r), None if g_const is None else g_const.reshape(S, d, 1)) if batched else \
                (g_beta.reshape(r), None if g_const is None else g_const.reshape(d, 1))
        loss = None
        if out is None:
            loss2 = torch.empty(S, 2, dtype=torch.float32, device=dev)
            grad = torch.empty(S, d, p, dtype=torch.float32, device=dev)
        else:
            loss2, grad = self._dev(out[0], "out"), self._dev(out[1], "out")
            loss = self._dev(out[2], "out") if len(out) > 2 and out[2] is not None else None
            if loss2.numel() != 2 * S or grad.numel() != S * d * p or (loss is not None and loss.numel() != S):
                raise SymodeError(f"out buffers hold {loss2.numel()} / {grad.numel()} elements, expected {2 * S} / {S * d * p} [/ {S}]")
        if ws is None:
            ws = self.workspace(dev, d, order, flags, S, n)
        inv = 1.0 / (n * d) if inv_count is None else float(inv_count)
        live = (0xFFFFFFFFFFFFFFFF if live is None else int(live)) & 0xFFFFFFFFFFFFFFFF
        args = (self._ptr(aug), self._ptr(linear_m), self._ptr(jgx), n_g, S, d, order, flags) + map_args + \
            (self._ptr(mask), live, inv, float(w_sym), self._ptr(loss2), self._ptr(loss), self._ptr(grad)) + extra + \
            (self._ptr(ws), ws.numel() * 8, self._stream(x))
        keep += [loss2, loss, grad, ws]
        loss2, grad = loss2.reshape(S, 2), grad.reshape(S, d, p)
        return "symode_loss_grad_reversed_linear_quad", args, keep, ((loss2, grad) if batched else (loss2[0], grad[0])) + mapped

    def loss_grad_reversed(self, x, dx, gx, jgx, xi, mask, order, flags=0, w_sym=1.0, inv_count=None, out=None, ws=None,
                           live_columns=None, linear_m=None, gram=None, aug=None, coef=None, coef_out=None, reduced=None):
        """The closure MSE + w_sym * reversed regulariser in ONE pass (x read once, Theta(x) shared by both terms).
        Shapes as loss_grad / symreg_reversed (jgx may be the compact table of a point-constant Jacobian, as there).
        Returns (loss2, grad): loss2 (S, 2) [or (2,)] = (mse, regulariser), grad = d(mse + w_sym * regulariser)/dXi
        (S, d, p) [or (d, p)].
        ``live_columns``: an int, bit k set = library column k may hold a coefficient (``CoefMap.live_mask``); with the compact
        table the call goes to the _live entry (symode.h): columns outside the set count as zero, their gradient is zero,
        and where the library has a kernel for the set it leaves their per-point work out.  None: every column.
        ``linear_m``: the float64 (S, 1, p, p) matrices of ``linear_action`` where it found g(x) = J x (jgx the compact table):
        the call goes to symode_loss_grad_reversed_linear, whose kernel reads neither g(x) nor evaluates Theta(g x) -- the
        same closure up to rounding, not bit for bit; where the library's launcher keeps the streamed kernels it is the
        call without ``linear_m``.
        ``gram``: with ``linear_m``, the float64 (S, 1, p, p) RAW sums G = sum_n Theta(x_n) Theta(x_n)^T of each problem over the
        points of this call (``aug_gram(x, dx, order)[..., :p, :p]``, contiguous): the call goes to
        symode_loss_grad_reversed_linear_gram, whose point loop carries the residual alone -- the regulariser and its gradient
        are a d p p fp64 product per problem.  loss2[:, 0] keeps its bits, the rest agrees up to rounding; where the
        launcher's table keeps the plain fold kernel, and with SYMODE_FOLD_GRAM=0, it is the call without ``gram``
        (``closure_gram(ws)`` tells).
        ``aug``: with ``linear_m``, in the place of ``gram``: the whole float64 (S, p+d, p+d) augmented Gram ``aug_gram(x, dx, order)``
        of the points of this call.  The call goes to symode_loss_grad_reversed_linear_quad, which has no point loop at all: the
        residual, too, is a quadratic form of the matrix (``closure_quad(ws)`` tells).  x, dx and gx give the shapes and are not
        read.  ``out`` may carry a third buffer, loss (S,), that receives mse + w_sym * regulariser.  The library refuses the call
        under SYMODE_CLOSURE_FOLD=0, SYMODE_FOLD_GRAM=0 or SYMODE_FOLD_RESID_GRAM=0 (``closure_quad_enabled()``): pass ``gram``.
        ``coef`` = (CoefMap, beta (S, r), const (S, d, 1) or None), with ``aug``: the launch forms Xi from the variables itself
        (``xi`` is not read; Q beta in fp64, one rounding to fp32) and also returns the gradient by the variables:
        (loss2, grad, g_beta (S, r), g_const (S, d, 1) or None).  ``coef_out`` = (xi_out or None, g_beta, g_const or None): buffers
        for these, xi_out (S, d, p) receiving the Xi the launch formed.
        ``reduced`` = (step, beta, const, alias[, x, dx, sym, Q, live]): the same closure as a prepared step on its reduced
        form (``quad_step_plan``; the last five name the operands of the step's key).  The call is handed on in the first
        statement, the tuple as it is, and nothing else is read or checked -- every other argument may be None; it enters here
        so that whatever wraps this method to watch the reversed closures (a timer, a trace) sees these steps too.  Returns
        (loss, g_beta, g_const); None where the library's switches refuse the step; STEP_STALE where the key moved; from the
        native plan also STEP_SLOW (an operand it does not take as it lies: call its ``slow``) or a positive error code of
        the launch (for ``_check``)."""
        if reduced is not None:
            return reduced[0](reduced)
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        if x.shape != dx.shape:
            raise SymodeError(f"x {tuple(x.shape)} and dx {tuple(dx.shape)} differ")
        rev = self._reversed_operands(x, gx, jgx, compact_ok=True)
        if aug is not None:
            if gram is not None:
                raise SymodeError("aug takes the place of gram")
            name, args, _, result = self._closure_quad_call(x, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, live_columns,
                                                            linear_m, aug, coef, coef_out)
            self._check(getattr(self.lib, name)(*args), name)
            return result
        if coef is not None or coef_out is not None:
            raise SymodeError("coef goes with aug")
        return self._closure(x, dx, rev, xi, mask, order, flags, w_sym, inv_count, out, ws, live_columns, linear_m, gram)

    def loss_grad_latent(self, z, dz, B, y, xi, mask, order, flags=0, w_pair=1.0, inv_count=None, out=None, ws=None):
        """The closure of the latent fit in ONE pass (symode_loss_grad_latent): z, dz, y (S, N, d) or (N, d), B (S, N, d, d)
        or (N, d, d) -- the operands of ``model_utils.latent_operands`` --, xi / mask (S, d, p) or (d, p).
        Returns (loss2, grad): loss2 (S, 2) [or (2,)] = (mean |h(z) - dz|^2, mean |B h(z) - y|^2), grad = d(loss2[0] + w_pair *
        loss2[1])/dXi (S, d, p) [or (d, p)].  ``xi`` / ``out`` / ``ws`` / ``inv_count`` as in loss_grad."""
        z, dz, B, y = self._dev(z, "z"), self._dev(dz, "dz"), self._dev(B, "B"), self._dev(y, "y")
        batched, S, n, d = self._problems(z)
        if dz.shape != z.shape or y.shape != z.shape or tuple(B.shape) != tuple(z.shape) + (d,):
            raise SymodeError(f"dz {tuple(dz.shape)} / y {tuple(y.shape)} / B {tuple(B.shape)} do not match z {tuple(z.shape)}")
        for name, t in (("dz", dz), ("B", B), ("y", y)):
            if t.device != z.device:
                raise SymodeError(f"{name} is on {t.device}, z on {z.device}: all tensors of one launch live on one device")
        xi, mask, p = self._coef(xi, mask, d, order, flags, S, pinned_ok=True)
        loss, grad, ws, inv = self._closure_prologue(z, S, n, d, p, order, flags, 2, out, ws, inv_count)
        self._check(self.lib.symode_loss_grad_latent(self._ptr(z), self._ptr(dz), self._ptr(B), self._ptr(y), S, n, d, order, flags,
                                                     self._ptr(xi), self._ptr(mask), inv, float(w_pair), self._ptr(loss),
                                                     self._ptr(grad), self._ptr(ws), ws.numel() * 8, self._stream(z)),
                    "symode_loss_grad_latent")
        loss, grad = loss.reshape(S, 2), grad.reshape(S, d, p)
        return (loss, grad) if batched else (loss[0], grad[0])

    def symreg_reversed_gram(self, x, gx, jgx, order, flags=0):
        """fp64 Gram matrix R of the reversed regulariser (raw sums over points and group elements, no 1/(N d)):
        x (N, d), gx (n_g, N, d), jgx (n_g, N, d, d) -> (d p, d p); or x (S, N, d), gx (S, n_g, N, d), jgx (S, n_g, N, d, d)
        -> (S, d p, d p).  Rows / columns in Xi's (d, p) row-major order: the regulariser is v^T R v / (N d), v = vec(Xi * M)."""
        x = self._dev(x, "x")
        gx, jgx, n_g, _ = self._reversed_operands(x, gx, jgx)
        batched, S, n, d = self._problems(x)
        p = self.lib_size(d, order, flags)
        need = self.lib.symode_symreg_reversed_gram_workspace_bytes(d, order, flags, n_g, S, n)
        if need == 0:
            raise SymodeError(f"symreg_reversed_gram does not support the library d={d} order={order} flags={flags}")
        ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
        gram = torch.empty(S, d * p, d * p, dtype=torch.float64, device=x.device)
        self._check(self.lib.symode_symreg_reversed_gram(self._ptr(x), self._ptr(gx), self._ptr(jgx), n_g, S, n, d, order, flags,
                                                         self._ptr(gram), self._ptr(ws), need, self._stream(x)),
                    "symode_symreg_reversed_gram")
        return gram if batched else gram[0]

    def symreg_reversed_gram_gather(self, x, gx, jgx, idx, order, flags=0):
        """R of S index subsets of ONE shared data set: x (N, d), gx (n_g, N, d), jgx (n_g, N, d, d), idx (S, M) int32 rows
        -> (S, d p, d p) fp64, bit-identical to ``symreg_reversed_gram`` on the materialised x[idx[s]], gx[:, idx[s]],
        jgx[:, idx[s]].  The kernel reads the table unchecked, so its range is checked here on EVERY call (one aminmax, one
        sync): a table refilled through a raw pointer or an alias keeps its version counter, so no verdict is remembered."""
        x, gx, jgx = self._dev(x, "x"), self._dev(gx, "gx"), self._dev(jgx, "jgx")
        idx = self._dev(idx, "idx", torch.int32)
        if x.dim() != 2 or gx.dim() != 3 or idx.dim() != 2:
            raise SymodeError("symreg_reversed_gram_gather expects x (N, d), gx (n_g, N, d), jgx (n_g, N, d, d) and idx (S, M)")
        n_src, d = x.shape
        n_g = gx.shape[0]
        S, m = idx.shape
        if n_g < 1 or tuple(gx.shape) != (n_g, n_src, d) or tuple(jgx.shape) != (n_g, n_src, d, d):
            raise SymodeError(f"gx {tuple(gx.shape)} / jgx {tuple(jgx.shape)} do not match x {tuple(x.shape)}")
        if S < 1 or m < 1:
            raise SymodeError(f"idx {tuple(idx.shape)} holds no rows")
        lo, hi = torch.stack(torch.aminmax(idx)).tolist()
        if lo < 0 or hi >= n_src:
            raise SymodeError("idx holds row indices outside [0, N)")
        p = self.lib_size(d, order, flags)
        need = self.lib.symode_symreg_reversed_gram_gather_workspace_bytes(d, order, flags, n_g, S, m)
        if need == 0:
            raise SymodeError(f"symreg_reversed_gram_gather does not support the library d={d} order={order} flags={flags}")
        ws = torch.empty(need // 8, dtype=torch.float64, device=x.device)
        gram = torch.empty(S, d * p, d * p, dtype=torch.float64, device=x.device)
        self._check(self.lib.symode_symreg_reversed_gram_gather(self._ptr(x), self._ptr(gx), self._ptr(jgx), n_g, n_src,
                                                                self._ptr(idx), S, m, d, order, flags, self._ptr(gram),
                                                                self._ptr(ws), need, self._stream(x)),
                    "symode_symreg_reversed_gram_gather")
        return gram

    def stlsq_sweep(self, G, n_points, gamma, threshold, max_iter, hyper=None, n_problems=None, *, d, near_band=1e-4, to_host=False,
                    tail=None):
        """Sequential-threshold least squares to convergence for every problem in ONE launch (symode_stlsq_sweep: the
        full-rank driver's loop of symode_host_stlsq_sweep on the device).  G (n_sets, p+d, p+d) fp64 on the device, ``d``
        the number of equation rows (G alone does not say where p ends).  ``hyper`` (n_problems, 2) fp32 on the device,
        row s = problem s's [gamma, threshold] on set s % n_sets (``gamma`` and ``threshold`` are then not read);
        ``n_problems`` defaults to the table's rows, or to n_sets without a table.
        Returns device tensors (Xi (n_problems, d, p) fp32, mask (n_problems, d, p) uint8, passes, near, fell (n_problems,)
        int32); a problem with ``fell`` set met a pivot that is not positive and is the host's to solve.  ``to_host=True``:
        the same five as numpy arrays, after one copy of the one buffer they share.  ``tail``: an int32 device tensor that
        rides in that buffer behind the five (a sixth item of the result), so that a caller with flags of its own to read
        fetches them in the same copy."""
        G = self._dev(G, "G", torch.float64)
        d = int(d)
        n_sets, p = self._stlsq_G(G, d)
        hyper, S = self._stlsq_hyper(hyper, n_problems, G, STLSQ_HYPER, "gamma, threshold")
        o, fetch = self._stlsq_outputs(G, "symode_stlsq_sweep", S, d, p, tail=tail)
        self._check(self.lib.symode_stlsq_sweep(self._ptr(G), n_sets, S, d, p, int(n_points), self._ptr(hyper), float(gamma),
                                                float(threshold), int(max_iter), float(near_band),
                                                *(o[k].data_ptr() for k in ("xi", "mask", "passes", "near", "fell")), self._stream(G)),
                    "symode_stlsq_sweep")
        return tuple(fetch(to_host).values())

    def gram_resample(self, chunk, seeds, n_replicas, want_counts=False):
        """Block-bootstrap replicas of Gram matrices in ONE launch (symode_gram_resample).  ``chunk`` (n_seeds, n_chunks, n, n) fp64
        on the device, the Gram matrices of every seed's chunks of rows; ``seeds`` (n_seeds,) int64 on the device, or a list of
        integers.  Returns (n_seeds * n_replicas, n, n) fp64 on the device, replica b of seed k at k * n_replicas + b: the sum of
        the seed's chunk matrices weighted by how often each of the n_chunks draws of (seed, b) landed on it.
        ``want_counts=True``: (replicas, counts (n_seeds * n_replicas, n_chunks) int32 on the device)."""
        chunk = self._dev(chunk, "chunk", torch.float64)
        if chunk.dim() != 4 or chunk.shape[2] != chunk.shape[3]:
            raise SymodeError(f"chunk must be (n_seeds, n_chunks, n, n), got {tuple(chunk.shape)}")
        if not isinstance(seeds, torch.Tensor):
            seeds = torch.tensor([int(v) for v in seeds], dtype=torch.int64).to(chunk.device)
        seeds = self._dev(seeds, "seeds", torch.int64)
        S, C, n, _ = chunk.shape
        if tuple(seeds.shape) != (S,) or seeds.device != chunk.device:
            raise SymodeError(f"seeds must be ({S},) int64 on {chunk.device}, got {tuple(seeds.shape)} on {seeds.device}")
        B = int(n_replicas)
        out = torch.empty(max(S * B, 0), n, n, dtype=torch.float64, device=chunk.device)
        counts = torch.empty(max(S * B, 0), C, dtype=torch.int32, device=chunk.device) if want_counts else None
        self._check(self.lib.symode_gram_resample(self._ptr(chunk), self._ptr(seeds), S, C, n, B, self._ptr(out), self._ptr(counts),
                                                  self._stream(chunk)), "symode_gram_resample")
        return (out, counts) if want_counts else out

    def stlsq_bag(self, G, rep_xi, rep_mask, rep_fell, n_replicas, gamma, tau_milli=1000, tau_table=None, *, d, to_host=False):
        """Aggregate the replica fits of every seed and refit on the terms kept, ONE launch (symode_stlsq_bag).  G (n_seeds, p+d,
        p+d) fp64 on the device, each seed's own matrix; ``rep_xi`` (n_seeds * n_replicas, d, p) fp32, ``rep_mask`` (same) uint8 and
        ``rep_fell`` (n_seeds * n_replicas,) int32 on the device: Xi, mask and fell of ``stlsq_sweep`` on ``gram_resample``'s
        matrices.  ``tau_milli``: the inclusion level in thousandths for all problems (one per seed); ``tau_table`` (n_problems,)
        int32 on the device or a list of integers: problem s is seed s % n_seeds at level tau_table[s], every value in 0 .. 1000
        (a list is checked here; a device tensor is the caller's to have checked).
        Returns (Xi (n_problems, d, p) fp32, mask (n_problems, d, p) uint8, fell (n_problems,) int32, count (n_seeds, d, p) int32,
        valid (n_seeds,) int32, mean, std (n_seeds, d, p) fp64) as device tensors; ``to_host=True``: numpy arrays after one copy
        of the one buffer they share."""
        G = self._dev(G, "G", torch.float64)
        d = int(d)
        n_seeds, p = self._stlsq_G(G, d)
        B = int(n_replicas)
        rep_xi, rep_mask = self._dev(rep_xi, "rep_xi"), self._dev(rep_mask, "rep_mask", torch.uint8)
        rep_fell = self._dev(rep_fell, "rep_fell", torch.int32)
        rows = n_seeds * max(B, 0)
        if tuple(rep_xi.shape) != (rows, d, p) or rep_mask.shape != rep_xi.shape or tuple(rep_fell.shape) != (rows,):
            raise SymodeError(f"rep_xi, rep_mask must be (n_seeds * n_replicas, d, p) = ({rows}, {d}, {p}) and rep_fell ({rows},), got "
                              f"{tuple(rep_xi.shape)}, {tuple(rep_mask.shape)}, {tuple(rep_fell.shape)}")
        if any(t.device != G.device for t in (rep_xi, rep_mask, rep_fell)):
            raise SymodeError(f"the replica outputs must lie on {G.device}")
        S = n_seeds
        if tau_table is not None:
            if not isinstance(tau_table, torch.Tensor):
                values = [int(v) for v in tau_table]
                if any(v < 0 or v > 1000 for v in values):
                    raise SymodeError(f"tau_table: every inclusion level must lie in 0 .. 1000 thousandths, got {values}")
                tau_table = torch.tensor(values, dtype=torch.int32).to(G.device)
            tau_table = self._dev(tau_table, "tau_table", torch.int32)
            if tau_table.dim() != 1 or tau_table.device != G.device:
                raise SymodeError(f"tau_table must be (n_problems,) int32 on {G.device}")
            S = tau_table.shape[0]
        o, fetch = self._stlsq_outputs(G, "symode_stlsq_bag", S, d, p)
        self._check(self.lib.symode_stlsq_bag(self._ptr(G), n_seeds, S, d, p, B, self._ptr(rep_xi), self._ptr(rep_mask),
                                              self._ptr(rep_fell), self._ptr(tau_table), int(tau_milli), float(gamma),
                                              *(o[k].data_ptr() for k in ("xi", "mask", "fell", "count", "valid", "mean", "std")),
                                              self._stream(G)), "symode_stlsq_bag")
        o = fetch(to_host)
        return tuple(o[k] for k in ("xi", "mask", "fell")) + tuple(o[k][:n_seeds] for k in ("count", "valid", "mean", "std"))

    def stlsq_path(self, G, V, n_points, gamma, tol, floor_rel, n_problems=None, *, d, near_band=1e-4, to_host=False,
                   keep_path=False):
        """The sparsity path of every problem in ONE launch (symode_stlsq_path): backward elimination from the full library to
        the empty model, every model scored on the held-out matrix, the sparsest one within ``tol`` of the best kept.  G
        (n_sets, p+d, p+d) and V (n_val_sets, p+d, p+d) fp64 on the device, raw sums of the training and the held-out rows;
        problem s reads sets s % n_sets and s % n_val_sets; ``n_problems`` defaults to n_sets.  ``gamma`` the ridge weight.
        Returns a dict of device tensors: Xi (n_problems, d, p) fp32, mask (n_problems, d, p) uint8, order (n_problems, d, p)
        int32, rss_train, rss_val (n_problems, d, p+1) fp64, best (n_problems, d), near, fell (n_problems,) int32 -- a problem
        with ``fell`` set met a pivot that is not positive and is the host's to solve -- and path_xi (n_problems, d, p+1, p)
        fp32.  ``to_host=True``: numpy arrays after ONE copy of the buffer the small outputs share; path_xi (the one large
        output) is then fetched only with ``keep_path=True`` and left out of the dict otherwise -- that saves its copy, not its
        allocation or the kernel's writes: the entry always writes the path."""
        G = self._dev(G, "G", torch.float64)
        V = self._dev(V, "V", torch.float64)
        d = int(d)
        n_sets, p = self._stlsq_G(G, d)
        self._stlsq_V(V, G)
        S = n_sets if n_problems is None else int(n_problems)
        o, fetch = self._stlsq_outputs(G, "symode_stlsq_path", S, d, p)
        path = torch.empty(max(S, 0), d, p + 1, p, dtype=torch.float32, device=G.device)
        self._check(self.lib.symode_stlsq_path(self._ptr(G), self._ptr(V), n_sets, V.shape[0], S, d, p, int(n_points), float(gamma),
                                               float(tol), float(floor_rel), float(near_band), self._ptr(path),
                                               *(o[k].data_ptr() for k in ("order", "rss_train", "rss_val", "best", "Xi", "mask", "near",
                                                                           "fell")), self._stream(G)),
                    "symode_stlsq_path")
        return self._with_path(fetch(to_host), path, to_host, keep_path)

    @staticmethod
    def _with_path(o, path, to_host, keep_path):
        """path_xi, the one large output of a path launch, beside the small ones: on the host it is fetched only when kept"""
        if not to_host:
            o = dict(o, path_xi=path)
        elif keep_path:
            o["path_xi"] = path.cpu().numpy()
        return o

    def stlsq_sweep_constrained(self, G, n_points, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, hyper=None,
                                n_problems=None, *, d, pivot_floor, near_band=1e-4, to_host=False, tail=None):
        """``stlsq_sweep`` under the equivariance constraint Xi = Q beta (+ const) in ONE launch
        (symode_stlsq_sweep_constrained): per pass one joint system in the r' = r + (d if allow_constant else 0) free
        parameters.  G, ``hyper``, ``n_problems``, ``d``, ``near_band``, ``to_host`` and ``tail`` as ``stlsq_sweep``; ``q_solve``
        (d p, r') fp64 and ``q_xi`` (d p, r) fp32 on the device (``CoefMap.solve_matrix()``, ``CoefMap.xi_matrix()``);
        ``pivot_floor``: a pivot that is not above this fraction of the first one flags the problem.
        Returns (Xi (n_problems, d, p) fp32 -- of the last solve, unmasked --, mask uint8, passes, near, fell int32, var
        (n_problems, r') fp32 = [beta | const]) and, behind them, the tail; a problem with ``fell`` set is possibly rank
        deficient and the host's to solve."""
        return self._stlsq_sweep_q("symode_stlsq_sweep_constrained", pivot_floor, (), G, n_points, gamma, threshold, max_iter, q_solve,
                                   q_xi, allow_constant, hyper, n_problems, d, near_band, to_host, tail)

    def _stlsq_sweep_q(self, entry, floor, more, G, n_points, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, hyper, n_problems,
                       d, near_band, to_host, tail):
        """The constrained launch and its rank-revealing mode: they differ by the entry, by what ``floor`` means (pivot_floor,
        rcond) and by the int32 outputs ``more`` behind var."""
        G = self._dev(G, "G", torch.float64)
        d = int(d)
        n_sets, p = self._stlsq_G(G, d)
        q_solve, q_xi, r, R = self._stlsq_Q(q_solve, q_xi, allow_constant, G, d, p)
        hyper, S = self._stlsq_hyper(hyper, n_problems, G, STLSQ_HYPER, "gamma, threshold")
        o, fetch = self._stlsq_outputs(G, entry, S, d, p, R, tail)
        self._check(getattr(self.lib, entry)(
            self._ptr(G), n_sets, S, d, p, int(n_points), self._ptr(q_solve), self._ptr(q_xi), r, 1 if allow_constant else 0,
            self._ptr(hyper), float(gamma), float(threshold), int(max_iter), float(near_band), float(floor),
            *(o[k].data_ptr() for k in ("xi", "var", "mask", "passes", "near", "fell") + more), self._stream(G)), entry)
        return tuple(fetch(to_host).values())

    def stlsq_sweep_minnorm(self, G, n_points, gamma, threshold, max_iter, q_solve, q_xi, allow_constant, hyper=None,
                            n_problems=None, *, d, rcond, near_band=1e-4, to_host=False, tail=None):
        """``stlsq_sweep_constrained`` in its rank-revealing mode, ONE launch (symode_stlsq_sweep_minnorm): every pass is solved
        as ``lstsq_normal(Gq, cq, m, 'gelsy', rcond)`` solves it on the host -- pivoted Cholesky without a pivot floor, the rank
        by xGELSY's loop over xLAIC1 estimates with ``rcond`` (the cut on the triangular factor), the minimum-norm solution
        where the rank is short -- so a problem whose support leaves Q's columns collinear ends inside the launch.  The other
        arguments as ``stlsq_sweep_constrained``.
        Returns (Xi, mask, passes, near, fell, var, trunc, rank) and, behind them, the tail: ``trunc`` (n_problems,) int32 the
        passes solved with rank < n, ``rank`` the rank of the last pass's system; ``fell`` is set only where the factor of
        Wm Wm^T met a diagonal that is not positive (the host's to solve)."""
        return self._stlsq_sweep_q("symode_stlsq_sweep_minnorm", rcond, ("trunc", "rank"), G, n_points, gamma, threshold, max_iter,
                                   q_solve, q_xi, allow_constant, hyper, n_problems, d, near_band, to_host, tail)

    def stlsq_sweep_symreg(self, G, R, n_points, gamma, threshold, w_sym, max_iter, hyper=None, n_problems=None, *, d, pivot_floor,
                           near_band=1e-4, to_host=False, tail=None):
        """``stlsq_sweep`` with the reversed symmetry regulariser in ONE launch (symode_stlsq_sweep_symreg): per pass the
        minimiser of mse + w_sym * reg on the support, one joint system in the n <= d p <= 64 active coefficients.  G,
        ``n_problems``, ``d``, ``near_band``, ``to_host`` and ``tail`` as ``stlsq_sweep``; R (n_sets, d p, d p) fp64 on the device
        (``symreg_reversed_gram(_gather)``: raw sums); ``hyper`` (n_problems, 3) fp32 on the device, row s = problem s's
        [gamma, threshold, w_sym]; ``pivot_floor`` as ``stlsq_sweep_constrained``.  The launch takes gamma, threshold and w_sym in
        fp32 with or without a table.
        Returns (Xi (n_problems, d, p) fp32 -- of the last solve, zeros off its support --, mask uint8, passes, near, fell int32)
        and, behind them, the tail; a problem with ``fell`` set is possibly rank deficient and the host's to solve."""
        G = self._dev(G, "G", torch.float64)
        d = int(d)
        n_sets, p = self._stlsq_G(G, d)
        R = self._dev(R, "R", torch.float64)
        self._stlsq_R(R, G, n_sets, d * p)
        hyper, S = self._stlsq_hyper(hyper, n_problems, G, STLSQ_SYMREG_HYPER, "gamma, threshold, w_sym")
        o, fetch = self._stlsq_outputs(G, "symode_stlsq_sweep_symreg", S, d, p, tail=tail)
        self._check(self.lib.symode_stlsq_sweep_symreg(
            self._ptr(G), self._ptr(R), n_sets, S, d, p, int(n_points), self._ptr(hyper), float(gamma), float(threshold), float(w_sym),
            int(max_iter), float(near_band), float(pivot_floor), *(o[k].data_ptr() for k in ("xi", "mask", "passes", "near", "fell")),
            self._stream(G)),
            "symode_stlsq_sweep_symreg")
        return tuple(fetch(to_host).values())

    def stlsq_path_symreg(self, G, R, V, n_points, gamma, w_sym, tol, floor_rel, hyper=None, n_problems=None, *, d, pivot_floor,
                          near_band=1e-4, to_host=False, keep_path=False):
        """``stlsq_path`` with the reversed symmetry regulariser in ONE launch (symode_stlsq_path_symreg): backward elimination
        over the JOINT (d, p) support of the minimiser of mse + w_sym * reg, n0 = d p <= 64 entries, from the full library to
        the empty model, every model scored on the held-out matrix, the sparsest one within ``tol`` of the best kept.  G, V,
        ``tol``, ``floor_rel``, ``near_band``, ``to_host`` and ``keep_path`` as ``stlsq_path``; R and ``pivot_floor`` as
        ``stlsq_sweep_symreg``; ``hyper`` (n_problems, 2) fp32 on the device, row s = problem s's [gamma, w_sym].  The launch
        takes gamma and w_sym in fp32 with or without a table.
        Returns a dict of device tensors, one chain per PROBLEM (not per equation row): Xi (n_problems, d, p) fp32, mask uint8,
        order (n_problems, n0) int32 flat indices j p + k, mse_train, reg_train, mse_val (n_problems, n0+1) fp64, best, near,
        fell (n_problems,) int32 -- a problem with ``fell`` set is possibly rank deficient and the host's to solve -- and
        path_xi (n_problems, n0+1, d, p) fp32 (with ``to_host=True`` only when ``keep_path``)."""
        G = self._dev(G, "G", torch.float64)
        V = self._dev(V, "V", torch.float64)
        R = self._dev(R, "R", torch.float64)
        d = int(d)
        n_sets, p = self._stlsq_G(G, d)
        self._stlsq_V(V, G)
        n0 = d * p
        self._stlsq_R(R, G, n_sets, n0)
        hyper, S = self._stlsq_hyper(hyper, n_problems, G, STLSQ_PATH_SYMREG_HYPER, "gamma, w_sym")
        o, fetch = self._stlsq_outputs(G, "symode_stlsq_path_symreg", S, d, p)
        path = torch.empty(max(S, 0), n0 + 1, d, p, dtype=torch.float32, device=G.device)
        self._check(self.lib.symode_stlsq_path_symreg(
            self._ptr(G), self._ptr(R), self._ptr(V), n_sets, V.shape[0], S, d, p, int(n_points), self._ptr(hyper), float(gamma),
            float(w_sym), float(tol), float(floor_rel), float(near_band), float(pivot_floor), self._ptr(path),
            *(o[k].data_ptr() for k in ("order", "mse_train", "reg_train", "mse_val", "best", "Xi", "mask", "near", "fell")),
            self._stream(G)),
            "symode_stlsq_path_symreg")
        return self._with_path(fetch(to_host), path, to_host, keep_path)

    def quad_closure(self, G, R, xi, mask, inv_count, w_sym=1.0, hyper=None, n_sets=None):
        """The closure as a quadratic form of fixed fp64 matrices: G (S, p+d, p+d) augmented Gram, R (S, d p, d p) or None,
        xi / mask (S, d, p) (mask may be None).  Returns what loss_grad (R None: loss (S,)) or loss_grad_reversed (loss2
        (S, 2)) returns, with grad (S, d, p); unbatched G (p+d, p+d) gives unbatched outputs.
        ``hyper`` (n_problems, 4) fp32 on the device, ``n_sets`` (default: G's sets): symode_quad_closure_grid -- xi / mask
        (n_problems, d, p), problem s on set s % n_sets with its w_sym from column 3 of row s (``w_sym`` is not read)."""
        batched = G.dim() == 3
        G = self._dev(G, "G", torch.float64).reshape(-1, G.shape[-2], G.shape[-1])
        n_mat, F = G.shape[0], G.shape[1]
        xi = self._dev(xi, "xi")
        d = xi.shape[-2]
        p = F - d
        S = n_mat
        if hyper is not None:
            n_sets = n_mat if n_sets is None else int(n_sets)
            hyper = self._dev(hyper, "hyper")
            if hyper.dim() != 2 or hyper.shape[1] != TRAINER_HYPER or n_sets != n_mat or hyper.shape[0] % n_sets != 0:
                raise SymodeError(f"hyper {tuple(hyper.shape)} must be (n_problems, {TRAINER_HYPER}) with n_problems a multiple of "
                                  f"the {n_mat} sets of matrices (n_sets {n_sets})")
            S = hyper.shape[0]
        elif n_sets is not None:
            raise SymodeError("n_sets goes with hyper (symode_quad_closure_grid)")
        if G.shape[2] != F or xi.numel() != S * d * p:
            raise SymodeError(f"G {tuple(G.shape)} and xi {tuple(xi.shape)} do not match")
        mask = None if mask is None else self._dev(mask, "mask")
        if mask is not None and mask.numel() != xi.numel():
            raise SymodeError("mask does not match xi")
        if R is not None:
            R = self._dev(R, "R", torch.float64)
            if R.numel() != n_mat * (d * p) ** 2:
                raise SymodeError(f"R {tuple(R.shape)} does not match ({n_mat}, {d * p}, {d * p})")
        loss = torch.empty(S, 2 if R is not None else 1, dtype=torch.float32, device=G.device)
        grad = torch.empty(S, d, p, dtype=torch.float32, device=G.device)
        if hyper is not None:
            self._check(self.lib.symode_quad_closure_grid(self._ptr(G), self._ptr(R), n_sets, S, d, p, self._ptr(xi), self._ptr(mask),
                                                          float(inv_count), self._ptr(hyper), self._ptr(loss), self._ptr(grad),
                                                          self._stream(G)), "symode_quad_closure_grid")
        else:
            self._check(self.lib.symode_quad_closure(self._ptr(G), self._ptr(R), S, d, p, self._ptr(xi), self._ptr(mask),
                                                     float(inv_count), float(w_sym), self._ptr(loss), self._ptr(grad),
                                                     self._stream(G)), "symode_quad_closure")
        loss = loss if R is not None else loss.reshape(S)
        if not batched:
            return loss[0], grad[0]
        return loss, grad

    def bind_closure(self, x, dx, xi, mask, order, flags, out, ws, stream, reversed_sym=None, w_sym=1.0):
        """A zero-argument callable that launches the single-problem closure on fixed buffers: every check and every
        ctypes conversion is done once, here (a latency-bound caller -- one L-BFGS closure is 8 us of GPU time -- pays
        ~15 us of Python per call otherwise).  ``out`` = (loss, grad) [(loss2, grad) with ``reversed_sym = (gx, jgx)``,
        materialised]; ``xi`` / ``out`` may be pinned host tensors; ``stream`` a torch stream.  The callable keeps the
        tensors alive."""
        x, dx = self._dev(x, "x"), self._dev(dx, "dx")
        if x.dim() != 2 or out is None or ws is None:
            raise SymodeError("a bound closure is one problem, x (N, d), on the caller's out buffers and private workspace")
        rev = None if reversed_sym is None else self._reversed_operands(x, *reversed_sym)
        name, args, keep, _ = self._closure_call(x, dx, rev, xi, mask, order, flags, w_sym, None, out, ws,
                                                 c_void_p(stream.cuda_stream))
        fn = getattr(self.lib, name)
        args = tuple(a if isinstance(a, t) else t(a) for t, a in zip(fn.argtypes, args))

        def launch(_fn=fn, _args=args, _keep=keep + (stream,)):
            rc = _fn(*_args)
            if rc != 0:
                self._check(rc, "bound closure")
        return launch

    def weak_gram(self, x, V, V_drv, order, flags=0):
        """Weak-SINDy contraction: x (T, d) one trajectory, V / V_drv (K, T) -> (G = V Theta(x) (K, p), b = -V_drv x (K, d)), fp64."""
        x, V, V_drv = self._dev(x, "x"), self._dev(V, "V"), self._dev(V_drv, "V_drv")
        if x.dim() != 2 or V.dim() != 2 or V.shape != V_drv.shape or V.shape[1] != x.shape[0]:
            raise SymodeError(f"weak_gram expects x (T, d) and V, V_drv (K, T); got {tuple(x.shape)}, {tuple(V.shape)}, {tuple(V_drv.shape)}")
        T, d = x.shape
        K = V.shape[0]
        p = self.lib_size(d, order, flags)
        R, C = 16 * ((2 * K + 15) // 16), 16 * ((p + d + 15) // 16)
        out = torch.empty(R, C, dtype=torch.float64, device=x.device)
        # room for the widest launch (64 time slabs x row tiles x column tiles of 256 fp64 partials behind the header):
        # a scratch sized for the closures alone made the library halve the grid to 5 workgroups at T = 10^4
        ws = self.workspace(x.device, d, order, flags, 1, T, min_bytes=8 * (8 + 32768 + 64 * (R // 16) * (C // 16) * 256) + 4096)
        self._check(self.lib.symode_weak_gram(self._ptr(x), T, d, order, flags, self._ptr(V), self._ptr(V_drv), K, self._ptr(out),
                                              self._ptr(ws), ws.numel() * 8, self._stream(x)), "symode_weak_gram")
        return out[:K, :p], out[K:2 * K, p:p + d]

    @staticmethod
    def check_windows(windows, n_ics, n_steps, n_t):
        """The (S, 2) int32 host table of ``weak_normal_windows``, or SymodeError naming the first row that is not
        [trajectory in [0, n_ics), start in [0, n_steps - n_t]].  Host arithmetic only."""
        import numpy as np
        w = np.asarray(windows)
        if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < 1 or not np.issubdtype(w.dtype, np.integer):
            raise SymodeError(f"windows must be a host integer array (S, 2) of [trajectory, start] rows, got {w.dtype} {w.shape}")
        if not 1 <= n_t <= n_steps:
            raise SymodeError(f"n_t = {n_t} must lie in 1 .. n_steps = {n_steps}")
        w = w.astype(np.int64)
        bad = (w[:, 0] < 0) | (w[:, 0] >= n_ics) | (w[:, 1] < 0) | (w[:, 1] > n_steps - n_t)
        if bad.any():
            s = int(np.argmax(bad))
            raise SymodeError(f"windows[{s}] = [{w[s, 0]}, {w[s, 1]}] is out of range: trajectory in [0, {n_ics}), start in "
                              f"[0, {n_steps - n_t}] for n_t = {n_t} of {n_steps} steps")
        return np.ascontiguousarray(w, dtype=np.int32)

    def weak_normal_windows(self, x, windows, n_t, V, V_drv, M, order, flags=0, want_z=False):
        """The normal matrices of the weak-SINDy fit for S windows of one data set in ONE call (symode_weak_normal_windows).
        x (n_ics, n_steps, d) fp32 on the device; ``windows`` (S, 2) host integers, row s = [trajectory, start], checked
        here (``check_windows``) before anything is uploaded or launched; V, V_drv (K, n_t) fp32 and M = V V^T (K, K) fp64
        on the device.  Returns (aug (S, p+d, p+d) fp64, bad (S,) int32) on the device, or (aug, z, bad) with
        ``want_z``: z (S, R, C) fp64, window s what ``symode_weak_gram`` writes for x[trajectory, start:start + n_t].
        No synchronisation: ``bad`` (the kernel's own range flags, all zero after the check here) is the caller's to
        fetch with its results."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise SymodeError("weak_normal_windows expects x (n_ics, n_steps, d)")
        return self._weak_normal_windows(x, self.check_windows(windows, x.shape[0], x.shape[1], int(n_t)), int(n_t), V, V_drv, M,
                                         order, flags, want_z)

    def _weak_normal_windows(self, x, w, n_t, V, V_drv, M, order, flags, want_z):
        """``weak_normal_windows`` behind its host check: ``w`` is the (S, 2) int32 table as the entry gets it."""
        n_ics, n_steps, d = x.shape
        x, V, V_drv, M = self._dev(x, "x"), self._dev(V, "V"), self._dev(V_drv, "V_drv"), self._dev(M, "M", torch.float64)
        K = V.shape[0]
        if V.dim() != 2 or V.shape != V_drv.shape or V.shape[1] != n_t or tuple(M.shape) != (K, K):
            raise SymodeError(f"weak_normal_windows expects V, V_drv (K, n_t = {n_t}) and M (K, K); got {tuple(V.shape)}, "
                              f"{tuple(V_drv.shape)}, {tuple(M.shape)}")
        S = w.shape[0]
        p = self.lib_size(d, order, flags)
        F, R, C = p + d, 16 * ((2 * K + 15) // 16), 16 * ((p + d + 15) // 16)
        win = torch.from_numpy(w).to(x.device)
        aug = torch.empty(S, F, F, dtype=torch.float64, device=x.device)
        z = torch.empty(S, R, C, dtype=torch.float64, device=x.device) if want_z else None
        bad = torch.empty(S, dtype=torch.int32, device=x.device)
        gx = min(64, (n_t + 255) // 256)
        # behind the header, every window's time-slab partials: the entry refuses a shorter scratch instead of halving gx
        ws = self.workspace(x.device, d, order, flags, 1, n_t, min_bytes=8 * (8 + 32768 + S * gx * (R // 16) * (C // 16) * 256) + 4096)
        self._check(self.lib.symode_weak_normal_windows(self._ptr(x), n_ics, n_steps, d, order, flags, self._ptr(win), S, n_t,
                                                        self._ptr(V), self._ptr(V_drv), K, self._ptr(M), self._ptr(aug),
                                                        self._ptr(z), self._ptr(bad), self._ptr(ws), ws.numel() * 8,
                                                        self._stream(x)), "symode_weak_normal_windows")
        return (aug, z, bad) if want_z else (aug, bad)

    def vjp(self, x, g, xi, mask, order, flags=0, need_grad_x=True):
        """Reverse mode of forward: returns (grad_x (N, d) or None, grad_xi (d, p))."""
        x, g = self._dev(x, "x"), self._dev(g, "g")
        n, d = x.shape[-2], x.shape[-1]
        xi, mask, p = self._coef(xi, mask, d, order, flags)
        gx = torch.empty_like(x) if need_grad_x else None
        gxi = torch.empty(d, p, dtype=torch.float32, device=x.device)
        ws = self.workspace(x.device, d, order, flags, 1, n)
        self._check(self.lib.symode_vjp(self._ptr(x), self._ptr(g), n, d, order, flags, self._ptr(xi), self._ptr(mask),
                                        self._ptr(gx), self._ptr(gxi), self._ptr(ws), ws.numel() * 8, self._stream(x)),
                    "symode_vjp")
        return gx, gxi

    def forward_jvp(self, x, v, xi, mask, order, flags=0, need_out=True):
        """Forward mode: (out, J.v) for tangents v of x's shape."""
        x, v = self._dev(x, "x"), self._dev(v, "v")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, _ = self._coef(xi, mask, d, order, flags)
        out = torch.empty_like(x) if need_out else None
        jv = torch.empty_like(x)
        self._check(self.lib.symode_forward_jvp(self._ptr(x), self._ptr(v), n, d, order, flags, self._ptr(xi),
                                                self._ptr(mask), self._ptr(out), self._ptr(jv), self._stream(x)),
                    "symode_forward_jvp")
        return out, jv


    def jvp_vjp(self, x, v, g_out, g_jv, xi, mask, order, flags=0):
        """Reverse mode of forward_jvp: returns (grad_x, grad_v, grad_xi); g_out may be None."""
        x, v, g_jv = self._dev(x, "x"), self._dev(v, "v"), self._dev(g_jv, "g_jv")
        g_out = None if g_out is None else self._dev(g_out, "g_out")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, p = self._coef(xi, mask, d, order, flags)
        gx, gv = torch.empty_like(x), torch.empty_like(x)
        gxi = torch.empty(d, p, dtype=torch.float32, device=x.device)
        ws = self.workspace(x.device, d, order, flags, 1, n)
        self._check(self.lib.symode_jvp_vjp(self._ptr(x), self._ptr(v), self._ptr(g_out), self._ptr(g_jv), n, d, order,
                                            flags, self._ptr(xi), self._ptr(mask), self._ptr(gx), self._ptr(gv),
                                            self._ptr(gxi), self._ptr(ws), ws.numel() * 8, self._stream(x)),
                    "symode_jvp_vjp")
        return gx, gv, gxi


    def rk4_traj(self, x0, xi, order, flags, n_steps, dt, subsample=1):
        """fp32 (x, dx) of shape (n_traj, ceil(n_steps/subsample), d): fp64 RK4 orbits of dx/dt = Theta(x) xi^T."""
        x0 = self._dev(x0, "x0", torch.float64)
        xi = self._dev(xi, "xi", torch.float64)
        n_traj, d = x0.shape
        p = self.lib_size(d, order, flags)
        if xi.shape != (d, p):
            raise SymodeError(f"xi must be ({d}, {p}), got {tuple(xi.shape)}")
        n_out = (n_steps + subsample - 1) // subsample
        x = torch.empty(n_traj, n_out, d, dtype=torch.float32, device=x0.device)
        dx = torch.empty_like(x)
        self._check(self.lib.symode_rk4_traj(self._ptr(x0), n_traj, d, order, flags, self._ptr(xi), int(n_steps), float(dt),
                                             int(subsample), self._ptr(x), self._ptr(dx), self._stream(x0)), "symode_rk4_traj")
        return x, dx

    def seeded_subsamples(self, n, m, seeds, device):
        """(len(seeds), m) int32 index table, rows ascending: per seed the m rows of range(n) with the smallest counter-based
        keys (symode_seeded_subsamples); depends on each seed alone."""
        s = torch.as_tensor([int(v) for v in seeds], dtype=torch.int64).to(device)
        out = torch.empty(len(s), int(m), dtype=torch.int32, device=s.device)
        self._check(self.lib.symode_seeded_subsamples(int(n), int(m), self._ptr(s), len(s), self._ptr(out), self._stream(out)),
                    "symode_seeded_subsamples")
        return out

    def euler_jvp(self, x, v, xi, mask, order, flags, n_steps, dt):
        """(f(x), J_f(x) v) for f = n_steps Euler steps of the regressor ODE; one launch."""
        x, v = self._dev(x, "x"), self._dev(v, "v")
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, _ = self._coef(xi, mask, d, order, flags)
        xo, to = torch.empty_like(x), torch.empty_like(x)
        self._check(self.lib.symode_euler_jvp(self._ptr(x), self._ptr(v), n, d, order, flags, self._ptr(xi), self._ptr(mask),
                                              int(n_steps), float(dt), self._ptr(xo), self._ptr(to), self._stream(x)),
                    "symode_euler_jvp")
        return xo, to

    def euler_jvp_vjp(self, x, v, g_x, g_t, xi, mask, order, flags, n_steps, dt):
        """Reverse mode of euler_jvp: (grad_x, grad_v, grad_xi)."""
        x, v, g_x, g_t = (self._dev(a, nm) for a, nm in ((x, "x"), (v, "v"), (g_x, "g_x"), (g_t, "g_t")))
        d = x.shape[-1]
        n = x.numel() // d
        xi, mask, p = self._coef(xi, mask, d, order, flags)
        gx, gv = torch.empty_like(x), torch.empty_like(x)
        gxi = torch.empty(d, p, dtype=torch.float32, device=x.device)
        ws = self.workspace(x.device, d, order, flags, 1, n)
        self._check(self.lib.symode_euler_jvp_vjp(self._ptr(x), self._ptr(v), self._ptr(g_x), self._ptr(g_t), n, d, order,
                                                  flags, self._ptr(xi), self._ptr(mask), int(n_steps), float(dt),
                                                  self._ptr(gx), self._ptr(gv), self._ptr(gxi), self._ptr(ws),
                                                  ws.numel() * 8, self._stream(x)), "symode_euler_jvp_vjp")
        return gx, gv, gxi

    def lbfgs_direction(self, g, old_dirs, old_stps, ro, head, count, h_diag):
        """d = -H g by the two-loop recursion for S problems at once (ring-buffered curvature pairs)."""
        g = self._dev(g, "g")
        S, n = g.shape
        H = old_dirs.shape[1]
        out = torch.empty_like(g)
        self._check(self.lib.symode_lbfgs_direction(self._ptr(g), self._ptr(self._dev(old_dirs, "old_dirs")),
                                                    self._ptr(self._dev(old_stps, "old_stps")), self._ptr(self._dev(ro, "ro")),
                                                    self._ptr(self._dev(head, "head", torch.int64)),
                                                    self._ptr(self._dev(count, "count", torch.int64)),
                                                    self._ptr(self._dev(h_diag, "h_diag")), S, n, H, self._ptr(out),
                                                    self._stream(g)), "symode_lbfgs_direction")
        return out

    def lbfgs_step(self, mode, new_loss, new_g, params, g, loss, act, st, lr, tol_grad, tol_change, l1=None, frozen=None):
        """In place: ONE launch for everything torch.optim.LBFGS.step does between two closure evaluations (``st``: the
        optimiser's state tensors, see sweep.BatchedLBFGS).  ``mode`` LBFGS_BEGIN opens an optimiser step (optimality test,
        first iteration up to the move; ``frozen`` (S,) bool: problems left untouched), LBFGS_ACCEPT finishes the running
        iteration of the problems with ``act`` set (stopping tests) and starts the next one; ``act`` (S,) bool out: moved.
        ``l1 = (w_x, w_reg)``: new_loss / new_g are the bare data term, the kernel forms w_x * loss + w_reg * |params|_1
        and its gradient.  The state tensors are checked in BEGIN, once per optimiser step."""
        S, n = params.shape
        new_loss, new_g = self._dev(new_loss, "new_loss"), self._dev(new_g, "new_g")
        if mode == LBFGS_BEGIN:
            for name, ten, dt in (("params", params, torch.float32), ("g", g, torch.float32), ("loss", loss, torch.float32),
                                  ("act", act, torch.bool), ("n_iter", st.n_iter, torch.int64), ("d", st.d, torch.float32),
                                  ("t", st.t, torch.float32), ("old_dirs", st.old_dirs, torch.float32),
                                  ("old_stps", st.old_stps, torch.float32), ("ro", st.ro, torch.float32),
                                  ("head", st.head, torch.int64), ("hist", st.hist, torch.int64),
                                  ("H_diag", st.H_diag, torch.float32), ("prev_g", st.prev_g, torch.float32),
                                  ("prev_loss", st.prev_loss, torch.float32), ("frozen", frozen, torch.bool)):
                if ten is not None and not (ten.is_cuda and ten.dtype == dt and ten.is_contiguous()):
                    raise SymodeError(f"lbfgs_step: {name} must be a contiguous {dt} GPU tensor")
            if new_loss.numel() != S or new_g.numel() != S * n or (frozen is not None and frozen.numel() != S):
                raise SymodeError("lbfgs_step: new_loss / frozen hold S values and new_g S * n for params (S, n)")
        w_x, w_reg = (1.0, 0.0) if l1 is None else l1
        self._check(self.lib.symode_lbfgs_step(
            int(mode), self._ptr(new_loss), self._ptr(new_g), self._ptr(frozen), float(tol_grad), 0 if l1 is None else 1, float(w_x),
            float(w_reg), self._ptr(params), self._ptr(g), self._ptr(loss), self._ptr(act), self._ptr(st.n_iter), self._ptr(st.d),
            self._ptr(st.t), self._ptr(st.old_dirs), self._ptr(st.old_stps), self._ptr(st.ro), self._ptr(st.head), self._ptr(st.hist),
            self._ptr(st.H_diag), self._ptr(st.prev_g), self._ptr(st.prev_loss), S, n, st.old_dirs.shape[1], float(lr),
            float(tol_change), self._stream(params)), "symode_lbfgs_step")


_ENGINE = None


def get_engine() -> HipEngine:
    """Process-wide engine; raises SymodeError if libsymode_hip.so is not built."""
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = HipEngine()
    return _ENGINE
