"""mbfir -- MI355X-native convex FIR / SLR beta-polynomial designer (host side).

Python mirror of the four convex designers of shanghong/Multiband-RF-pulse-Design
(same names, argument order, defaults, return convention and error behaviour as the
MATLAB functions they replace):

    h, status = fir_ap_cvx(n, f, a, d, obj, Peak, dbg)      # reference fir_ap_cvx.m:1
    h, status = fir_qp_cvx(n, f, a, d, k, obj, dbg)         # reference fir_qp_cvx.m:1
    h, status = fir_linprog(n, f, a, d, h0, dbg)            # reference ss/fir_linprog.m:2
    h, status = fir_qprog_phs(n, f, ac, dc, x0, dbg)        # reference ss/fir_qprog_phs.m:1

Everything is computed by the hand-written HIP solver behind the C ABI of
include/mbfir.h (libmbfir.so, built in-tree by __graft_entry__.build()); this module is
a ctypes binding plus argument checking.  There is NO CPU fallback: if the library is
missing or no GPU is present the calls raise.

The directory name contains '-', so import the package through the repo-root shim:
    import mbfir
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmbfir.so")

SOLVED, INFEASIBLE, NUMERICAL, EARLY_FAIL = 0, 1, 2, 3
E_ARG, E_HIP, E_NODEVICE = -1, -2, -3


class MbfirError(RuntimeError):
    pass


class Opts(C.Structure):
    """struct mbfir_opts (include/mbfir.h)."""
    _fields_ = [("grid_m", C.c_int), ("max_iter", C.c_int), ("feastol", C.c_double),
                ("abstol", C.c_double), ("reltol", C.c_double), ("refine", C.c_int),
                ("verbose", C.c_int), ("shard_rank", C.c_int), ("shard_size", C.c_int),
                ("dense_trig", C.c_int), ("ddkkt", C.c_int), ("lanes", C.c_int)]


class Info(C.Structure):
    """struct mbfir_info (include/mbfir.h)."""
    _fields_ = [("status", C.c_int), ("iters", C.c_int), ("n_unknowns", C.c_int), ("n_rows", C.c_int),
                ("n_freq", C.c_int), ("n_lp", C.c_int), ("n_q3", C.c_int), ("n_big", C.c_int),
                ("pcost", C.c_double), ("dcost", C.c_double), ("gap", C.c_double), ("relgap", C.c_double),
                ("pres", C.c_double), ("dres", C.c_double),
                ("ms_assemble", C.c_double), ("ms_solve", C.c_double), ("ms_post", C.c_double),
                ("ms_total", C.c_double), ("ms_gram", C.c_double), ("ms_chol", C.c_double),
                ("gram_flop", C.c_double), ("gram_launches", C.c_int), ("lattice", C.c_int),
                ("chol_flop", C.c_double), ("chol_launches", C.c_int), ("builds", C.c_int),
                ("dd_iters", C.c_int), ("dd_kmax", C.c_int), ("collectives", C.c_int), ("lanes", C.c_int),
                ("dd_form", C.c_int), ("ms_cap", C.c_double), ("cap_flop", C.c_double),
                ("collective_bytes", C.c_double), ("correctors", C.c_int), ("correctors_taken", C.c_int),
                ("gv_passes", C.c_int), ("gtv_passes", C.c_int), ("pair_passes", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Job(C.Structure):
    """struct mbfir_job (include/mbfir.h)."""
    _fields_ = [("which", C.c_int), ("n", C.c_int), ("nband", C.c_int), ("rc", C.c_int),
                ("f", C.POINTER(C.c_double)), ("a", C.POINTER(C.c_double)), ("d", C.POINTER(C.c_double)),
                ("params", C.c_double * 4), ("h_re", C.POINTER(C.c_double)), ("h_im", C.POINTER(C.c_double)),
                ("info", Info), ("z", C.POINTER(C.c_double)), ("z_cap", C.c_int), ("err", C.c_char * 128)]


class RemezJob(C.Structure):
    """struct mbfir_remez_job (include/mbfir.h)."""
    _fields_ = [("numtaps", C.c_int), ("nband", C.c_int), ("type", C.c_int), ("edges", C.POINTER(C.c_double)),
                ("desired", C.POINTER(C.c_double)), ("weight", C.POINTER(C.c_double)), ("h", C.POINTER(C.c_double)),
                ("ext", C.POINTER(C.c_double)), ("status", C.c_int), ("iterations", C.c_int), ("delta", C.c_double)]


class RemezOpts(C.Structure):
    """struct mbfir_remez_opts (include/mbfir.h)."""
    _fields_ = [("grid_density", C.c_int), ("maxiter", C.c_int)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_long)
_lib = None

# every symbol include/mbfir.h declares: name -> (restype, argtypes)
# the context and the forward arguments of the Bloch calls, up to the scale list
_BLOCH_HEAD = [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, _dp, _dp,
               C.c_int, _dp]
# the train's fused calls through ebcast: the Bloch head, the train's tables, demod, m0 and ebcast
_TRAIN_HEAD = _BLOCH_HEAD + [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int]
SYMBOLS = {
    "mbfir_create": (C.c_void_p, [C.c_int]),
    "mbfir_destroy": (None, [C.c_void_p]),
    "mbfir_last_error": (C.c_char_p, [C.c_void_p]),
    "mbfir_default_opts": (None, [C.POINTER(Opts)]),
    "mbfir_set_allreduce": (None, [C.c_void_p, ALLREDUCE_FN, C.c_void_p]),
    "mbfir_version": (C.c_char_p, []),
    "mbfir_comm_unique_id": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mbfir_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "mbfir_comm_destroy": (None, [C.c_void_p]),
    "mbfir_test_comm_allreduce": (C.c_int, [C.c_void_p, _dp, C.c_long, C.c_int]),
    "mbfir_last_solution": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "mbfir_ap_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double,
                                 C.POINTER(Opts), _dp, _dp, C.POINTER(Info)]),
    "mbfir_qp_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, _dp, C.c_int,
                                 C.POINTER(Opts), _dp, _dp, C.POINTER(Info)]),
    "mbfir_linprog_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp,
                                      C.POINTER(Opts), _dp, _dp, C.POINTER(Info)]),
    "mbfir_qprog_phs_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp,
                                        C.POINTER(Opts), _dp, _dp, C.POINTER(Info)]),
    "mbfir_solve_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Job), C.c_int, C.POINTER(Opts)]),
    "mbfir_b2a": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_ab2rf": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_b2rf": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_b2rf_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_slr2d_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int]),
    "mbfir_abr2": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_flip_search": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_long, C.POINTER(C.c_uint), _ip,
                                    C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_long), _dp]),
    "mbfir_test_flip_stages": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_long, C.POINTER(C.c_uint), _ip,
                                         C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _lp, _dp, _dp, _lp,
                                         _dp, _dp, _lp, _dp] + [_dp] * 8 + [_lp]),
    "mbfir_remez_batch": (C.c_int, [C.c_void_p, C.POINTER(RemezJob), C.c_int, C.POINTER(RemezOpts)]),
    "mbfir_fmp": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_abr": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_bloch": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, _dp, C.c_int,
                              _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp]),
    "mbfir_bloch_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp,
                                    C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]),
    "mbfir_abr_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp,
                                  _dp]),
    "mbfir_abr2_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int, _dp,
                                   C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_abr_vjp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, _dp, _dp,
                                      _dp, _dp, _dp, _dp]),
    "mbfir_abr2_vjp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int,
                                       _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_bloch_vjp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp,
                                        C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 11),
    "mbfir_bloch_vjp_gr_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                           _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 15),
    "mbfir_bloch_jvp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp,
                                        C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 3 + [C.c_int] + [_dp] * 11),
    "mbfir_test_bloch_jvp_group": (C.c_int, []),
    "mbfir_bloch_ss_vjp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                           _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 8),
    "mbfir_bloch_ss_jvp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                           _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [C.c_int] + [_dp] * 8),
    "mbfir_test_bloch_ss_jvp_group": (C.c_int, []),
    "mbfir_bloch_train_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                          _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                         [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 9),
    "mbfir_bloch_prop_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                         _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_ip] + [_dp] * 4),
    "mbfir_bloch_train_vjp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                              _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                             [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 14),
    "mbfir_bloch_train_vjp_gr_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                                 _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 18),
    "mbfir_bloch_train_vjp_sched_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int,
                                                    _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                   [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 14),
    "mbfir_bloch_train_jvp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                              _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                             [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] + [_dp] * 17),
    "mbfir_test_bloch_train_jvp_group": (C.c_int, [C.c_int]),
    "mbfir_bloch_train_jvp_sched_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int,
                                                    _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                   [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] +
                                                   [_dp] * 17),
    "mbfir_test_bloch_train_sched_jvp_group": (C.c_int, []),
    "mbfir_bloch_train_lsq_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                              _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                             [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] + [_dp] * 19),
    "mbfir_bloch_train_gn_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                              _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                             [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] + [_dp] * 7 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_train_lsq_sched_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int,
                                                    _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                   [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] +
                                                   [_dp] * 19),
    "mbfir_bloch_train_gn_sched_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int,
                                                   _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                  [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] +
                                                  [_dp] * 7 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_ss_vjp_gr_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                              _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 12),
    "mbfir_bloch_ss_lsq_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                           _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 12),
    "mbfir_bloch_ss_gn_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                          _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 3 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_lsq_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp,
                                        C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 12),
    "mbfir_bloch_gn_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp,
                                       C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 6 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_lm_step_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                            _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 9 + [C.c_int, C.c_double] +
                                           [_dp] * 5 + [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_bloch_ss_lm_step_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp,
                                               _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] + [_dp] * 6 + [C.c_int, C.c_double] +
                                              [_dp] * 5 + [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    # the magnitude twins: the pairs (wxy, wz) and (txy, tz) where the calls above take triples
    "mbfir_bloch_lsq_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 10),
    "mbfir_bloch_gn_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 5 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_ss_lsq_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 10),
    "mbfir_bloch_ss_gn_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 2 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_lm_step_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 8 + [C.c_int, C.c_double] + [_dp] * 4 +
                                      [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_bloch_ss_lm_step_mag_batch": (C.c_int, _BLOCH_HEAD + [_dp] * 5 + [C.c_int, C.c_double] + [_dp] * 4 +
                                         [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_bloch_train_lm_step_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, C.c_int,
                                                  _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                 [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] + [_dp] * 7 +
                                                 [_dp] * 3 + [C.c_int, C.c_double] + [_dp] * 8 + [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_bloch_train_lm_step_sched_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp,
                                                        C.c_int, _lp, _dp, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _dp] +
                                                       [_ip, _lp, _dp, _dp, _ip, _lp, _dp, _ip, _dp, C.c_int] + [_dp] * 3 + [C.c_int] +
                                                       [_dp] * 16 + [C.c_int, C.c_double] + [_dp] * 2 + [_ip, _dp, _dp, _ip] + [_dp] * 3),
    # the train's magnitude twins: pairs where the six train calls above take triples
    "mbfir_bloch_train_lsq_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 15),
    "mbfir_bloch_train_gn_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 5 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_train_lsq_sched_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 15),
    "mbfir_bloch_train_gn_sched_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 5 + [C.c_int] + [_dp] * 4),
    "mbfir_bloch_train_lm_step_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 5 + [_dp] * 3 + [C.c_int, C.c_double] + [_dp] * 6 +
                                            [_ip, _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_bloch_train_lm_step_sched_mag_batch": (C.c_int, _TRAIN_HEAD + [_dp] * 12 + [C.c_int, C.c_double] + [_dp] * 2 +
                                                  [_ip, _dp, _dp, _ip] + [_dp] * 3),
    "mbfir_abr_vjp_rfg_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, _dp,
                                          _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr2_vjp_rfg_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp,
                                           C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr_jvp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp,
                                      _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr2_jvp_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int,
                                       _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr_lsq_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp,
                                      _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr2_lsq_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int,
                                       _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbfir_abr_gn_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp,
                                     C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_abr2_gn_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int,
                                      _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "mbfir_abr_lm_step_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _dp, C.c_int, C.c_int,
                                          _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _dp, _dp,
                                          _dp]),
    "mbfir_abr2_lm_step_batch": (C.c_int, [C.c_void_p, C.c_int, _lp, _dp, _dp, _dp, _dp, C.c_int, _lp, _dp, C.c_int, _lp, _dp, C.c_int,
                                           _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip,
                                           _dp, _dp, _ip, _dp, _dp, _dp]),
    "mbfir_test_jvp_group": (C.c_int, []),
    "mbfir_test_sim_blocks": (C.c_long, [C.c_int, _ip, _lp, C.c_int, _ip]),
    "mbfir_assemble": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int,
                                 C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    "mbfir_program_free": (None, [C.c_void_p]),
    "mbfir_program_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mbfir_program_dims": (None, [C.c_void_p, _ip]),
    "mbfir_program_trig": (None, [C.c_void_p, _dp, _ip, _dp, _dp, _ip, _dp, _dp]),
    "mbfir_program_rows": (None, [C.c_void_p, _ip, _ip, _dp, _dp, _dp, _dp]),
    "mbfir_program_replicated": (None, [C.c_void_p, _ip]),
    "mbfir_test_gram": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]),
    "mbfir_test_chol": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "mbfir_test_chol_lanes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _dp, _dp, _dp]),
    "mbfir_test_specfact": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "mbfir_test_specfact_stages": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_long, _lp, _dp]),
    "mbfir_test_unit_ops": (C.c_int, [C.c_void_p, C.POINTER(Job), C.c_int, C.POINTER(Opts), C.c_int, C.c_int, C.c_int, C.c_int,
                                      _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _lp, _dp]),
    "mbfir_test_unit_cone": (C.c_int, [C.c_void_p, C.POINTER(Job), C.c_int, C.POINTER(Opts), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _lp]),
    "mbfir_test_unit_kkt": (C.c_int, [C.c_void_p, C.POINTER(Job), C.c_int, C.POINTER(Opts)] + [C.c_int] * 9 + [_ip, _ip] + [_dp] * 6 +
                                     [_dp, _dp, _dp, _dp, _lp, _dp, _dp, _dp, _dp, _dp, _dp, _lp]),
    "mbfir_test_unit_ddkkt": (C.c_int, [C.c_void_p, C.POINTER(Job), C.c_int, C.POINTER(Opts)] + [C.c_int] * 8 + [_ip] + [_dp] * 8 + [_ip, _ip] +
                                       [_dp] * 9 + [_lp] + [_dp] * 6 + [_lp, _lp]),
    "mbfir_test_fold": (C.c_int, [_dp, C.c_int, C.c_int, C.POINTER(C.c_long)]),
    "mbfir_test_ddsolve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip, _dp, _dp]),
    "mbfir_test_ddstages": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int,
                                      _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "mbfir_test_capsolve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp,
                                      _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "mbfir_test_mfma_peak": (C.c_int, [C.c_void_p, _dp, _dp]),
    "mbfir_test_time_kernels": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
}


def load_library():
    """dlopen libmbfir.so and bind every symbol of include/mbfir.h.  Raises when the
    library has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (same SONAME as /opt/rocm's).  Whichever is loaded first serves
    # the whole process, and torch stops seeing the GPU when it is not its own -- so load torch first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise MbfirError("libmbfir.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`"
                         % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _vec(x, dtype=np.float64):
    return np.ascontiguousarray(np.asarray(x, dtype=dtype).ravel())


def _ptr(a):
    return a.ctypes.data_as(_dp)


class Context:
    """Owns the device memory, stream and (optionally) the all-reduce hook of one GPU.
    Reusable across calls; not thread-safe (mirrors mbfir_ctx)."""

    def __init__(self, device=None):
        lib = load_library()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = device
        self._h = lib.mbfir_create(device)
        if not self._h:
            raise MbfirError("mbfir_create(%d) failed: %s" % (device, lib.mbfir_last_error(None).decode()))
        self._cb = None

    def close(self):
        if getattr(self, "_h", None):
            load_library().mbfir_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return load_library().mbfir_last_error(self._h).decode()

    def last_solution(self, n_unknowns):
        """Conic solution [x ; y] / tau of the last solve (mbfir_last_solution)."""
        z = np.zeros(int(n_unknowns))
        k = load_library().mbfir_last_solution(self._h, _ptr(z), len(z))
        if k < 0:
            raise MbfirError("mbfir_last_solution failed")
        return z[:k]

    def set_allreduce(self, fn):
        """fn(ptr:int, count:int, op:int) -> int ; op 0 = sum, 1 = max (device pointer).  An exception inside the
        hook is logged and reported as a failed collective (the solve then raises) instead of being swallowed by
        ctypes with an undefined return value."""
        def cb(buf, count, op, user):
            try:
                return int(fn(buf, count, op))
            except BaseException:                          # noqa: BLE001 -- must not propagate into C
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(cb)
        load_library().mbfir_set_allreduce(self._h, self._cb, None)

    def init_comm(self, rank=None, size=None, group=None):
        """Native RCCL communicator for row-sharded solves: rank 0 makes the unique id, torch.distributed (any
        backend) carries its 128 bytes to the other ranks, every rank joins (mbfir_comm_init).  From then on the
        solver issues its all-reduces itself, on its own stream."""
        import torch
        import torch.distributed as dist
        lib = load_library()
        # one RCCL per process: point the library at the copy torch has loaded
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(cand):
            os.environ.setdefault("MBFIR_RCCL_PATH", cand)
        rank = dist.get_rank(group) if rank is None else rank
        size = dist.get_world_size(group) if size is None else size
        buf = C.create_string_buffer(128)
        if rank == 0:
            _check(self, lib.mbfir_comm_unique_id(self._h, buf))
        box = [bytes(buf.raw)]
        if size > 1:
            dist.broadcast_object_list(box, src=0, group=group)
        _check(self, lib.mbfir_comm_init(self._h, int(size), int(rank), box[0]))

    def comm_allreduce(self, v, op=0):
        """test hook: all-reduce a host array through the context's RCCL communicator (in place)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        _check(self, load_library().mbfir_test_comm_allreduce(self._h, _ptr(v), v.size, int(op)))
        return v

    def destroy_comm(self):
        load_library().mbfir_comm_destroy(self._h)


class _DevArray:
    """__cuda_array_interface__ view of `count` doubles at a raw device pointer."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


def device_tensor(ptr, count):
    """torch tensor aliasing device memory owned by the solver (zero copy)."""
    import torch
    return torch.as_tensor(_DevArray(ptr, count), device="cuda")


def make_torch_allreduce(group=None, wrap=None):
    """All-reduce hook for row-sharded solves: fn(ptr, count, op) over torch.distributed
    (backend nccl = RCCL over xGMI; op 0 = sum, 1 = max).  `wrap(ptr, count)` makes the tensor
    (default: a zero-copy view of the device pointer); the hook returns once the result is in place."""
    import torch
    import torch.distributed as dist
    wrap = wrap or device_tensor

    def hook(ptr, count, op):
        t = wrap(ptr, count)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)
        if t.is_cuda:
            torch.cuda.current_stream().synchronize()
        return 0

    return hook


_default_ctx = {}


def get_context(device=None):
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def make_opts(**kw):
    o = Opts()
    load_library().mbfir_default_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown option %r" % k)
        setattr(o, k, v)
    return o


def opts_with(opts, **kw):
    """a copy of `opts` (None: the defaults) with the given fields replaced"""
    o = make_opts()
    if opts is not None:
        C.memmove(C.byref(o), C.byref(opts), C.sizeof(Opts))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown option %r" % k)
        setattr(o, k, v)
    return o


def _finish(ctx, rc, hre, him, info, want_info):
    if rc < 0:
        msg = ctx.last_error()
        if rc == E_ARG:
            raise ValueError(msg)            # the reference's error() calls
        raise MbfirError("mbfir solve failed (%d): %s" % (rc, msg))
    if rc == SOLVED:
        h, status = hre + 1j * him, "Solved"
    else:
        h, status = np.zeros(0, dtype=np.complex128), "Failed"      # h = [] on failure
    if want_info:
        d = info.as_dict()
        d["rc"] = rc
        return h, status, d
    return h, status


def fir_ap_cvx(n, f, a, d, obj=0.0, Peak=1e-3, dbg=0, *, opts=None, ctx=None, info=False):
    """Arbitrary-phase multiband magnitude design (reference fir_ap_cvx.m).
    Returns (h, status): h complex ndarray of n taps (the reference's 1 x n row),
    status 'Solved' or 'Failed' (h empty).  obj < 0 raises ValueError('invalid input of obj')."""
    if n is None or f is None or a is None or d is None:
        raise ValueError("not enough input")                       # fir_ap_cvx.m:32
    ctx = ctx or get_context()
    f, a, d = _vec(f), _vec(a), _vec(d)
    _check_spec(f, a, d)
    hre, him, inf = np.zeros(n), np.zeros(n), Info()
    o = opts if opts is not None else make_opts(verbose=1 if dbg else 0)
    rc = load_library().mbfir_ap_solve(ctx._h, int(n), len(d), _ptr(f), _ptr(a), _ptr(d), float(obj),
                                       float(Peak), C.byref(o), _ptr(hre), _ptr(him), C.byref(inf))
    return _finish(ctx, rc, hre, him, inf, info)


def fir_qp_cvx(n, f, a, d, k=100.0, obj=0.0, dbg=0, *, opts=None, ctx=None, info=False):
    """Quadratic-phase design (reference fir_qp_cvx.m).  obj scalar -> E_total + obj*Peak,
    two entries -> delta + obj(1)*E_total + obj(2)*Peak.  Returns (h, status), h n x 1."""
    if n is None or f is None or a is None or d is None:
        raise ValueError("not enough input")                       # fir_qp_cvx.m:28
    ctx = ctx or get_context()
    f, a, d = _vec(f), _vec(a), _vec(d)
    _check_spec(f, a, d)
    objv = _vec(obj)
    if len(objv) not in (1, 2):
        raise ValueError("invalid input of obj")                   # fir_qp_cvx.m:194-196
    hre, him, inf = np.zeros(n), np.zeros(n), Info()
    o = opts if opts is not None else make_opts(verbose=1 if dbg else 0)
    rc = load_library().mbfir_qp_solve(ctx._h, int(n), len(d), _ptr(f), _ptr(a), _ptr(d), float(k),
                                       _ptr(objv), len(objv), C.byref(o), _ptr(hre), _ptr(him), C.byref(inf))
    return _finish(ctx, rc, hre, him, inf, info)


def fir_linprog(n, f, a, d, h0=None, dbg=0, *, opts=None, ctx=None, info=False):
    """Linear-phase (Hermitian-symmetric) multiband LP (reference ss/fir_linprog.m).
    h0 is the reference's warm start for its active-set linprog; an interior-point
    method has no use for it and it is ignored.  Returns (h, status), h n x 1."""
    ctx = ctx or get_context()
    f, a, d = _vec(f), _vec(a), _vec(d)
    _check_spec(f, a, d)
    hre, him, inf = np.zeros(n), np.zeros(n), Info()
    o = opts if opts is not None else make_opts(verbose=1 if dbg else 0)
    rc = load_library().mbfir_linprog_solve(ctx._h, int(n), len(d), _ptr(f), _ptr(a), _ptr(d), C.byref(o),
                                            _ptr(hre), _ptr(him), C.byref(inf))
    return _finish(ctx, rc, hre, him, inf, info)


def fir_qprog_phs(n, f, ac, dc, x0=None, dbg=0, *, opts=None, ctx=None, info=False):
    """Minimum-energy design with per-band magnitude and phase bounds (reference
    ss/fir_qprog_phs.m).  ac (2 per band) and dc (1 per band) are complex.  x0 is
    overwritten by [] in the reference (:338) and ignored here.  Returns (h, status)."""
    ctx = ctx or get_context()
    f = _vec(f)
    ac = np.ascontiguousarray(np.asarray(ac, dtype=np.complex128).ravel())
    dc = np.ascontiguousarray(np.asarray(dc, dtype=np.complex128).ravel())
    if len(f) % 2 or len(ac) != len(f) or len(dc) != len(f) // 2:
        raise ValueError("f, ac, dc have inconsistent lengths")
    are, aim = _vec(ac.real), _vec(ac.imag)
    dre, dim = _vec(dc.real), _vec(dc.imag)
    hre, him, inf = np.zeros(n), np.zeros(n), Info()
    o = opts if opts is not None else make_opts(verbose=1 if dbg else 0)
    rc = load_library().mbfir_qprog_phs_solve(ctx._h, int(n), len(dc), _ptr(f), _ptr(are), _ptr(aim), _ptr(dre),
                                              _ptr(dim), C.byref(o), _ptr(hre), _ptr(him), C.byref(inf))
    return _finish(ctx, rc, hre, him, inf, info)


# ---- inverse SLR: beta polynomial -> alpha -> RF (dzrf_mb.m:239-244) -------------------------------
def _split(z):
    z = np.asarray(z, dtype=np.complex128).ravel()
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def b2a(bc, *, ctx=None):
    """`aca = b2a(bc)` (b2a.m:15): the minimum-phase alpha polynomial consistent with beta."""
    ctx = ctx or get_context()
    bre, bim = _split(bc)
    are, aim = np.zeros(len(bre)), np.zeros(len(bre))
    _check(ctx, load_library().mbfir_b2a(ctx._h, len(bre), _ptr(bre), _ptr(bim), _ptr(are), _ptr(aim)))
    return are + 1j * aim


def ab2rf(ac, bc, *, ctx=None):
    """`rf = ab2rf(ac, bc)` (ab2rf.m:14): inverse SLR transform, rf in radians per sample."""
    ctx = ctx or get_context()
    are, aim = _split(ac)
    bre, bim = _split(bc)
    if len(are) != len(bre):
        raise ValueError("ab2rf: alpha and beta must have the same length")
    rre, rim = np.zeros(len(bre)), np.zeros(len(bre))
    _check(ctx, load_library().mbfir_ab2rf(ctx._h, len(bre), _ptr(are), _ptr(aim), _ptr(bre), _ptr(bim),
                                           _ptr(rre), _ptr(rim)))
    return rre + 1j * rim


def b2rf(bc, *, ctx=None):
    """`rf = b2rf(bc)` = ab2rf(b2a(bc), bc) with alpha kept on the device (rf_tools/mex5/b2rf.c)."""
    ctx = ctx or get_context()
    bre, bim = _split(bc)
    rre, rim = np.zeros(len(bre)), np.zeros(len(bre))
    _check(ctx, load_library().mbfir_b2rf(ctx._h, len(bre), _ptr(bre), _ptr(bim), _ptr(rre), _ptr(rim)))
    return rre + 1j * rim


def b2rf_batch(B, *, ctx=None):
    """`rf(q, :) = b2rf(B(q, :))` for every row of a (count, n) array in one device launch (mbfir_b2rf_batch), 2 <= n <= 2048.
    Agrees with b2rf row by row to rounding; a row's result does not depend on the rest of the batch."""
    B = np.asarray(B, dtype=np.complex128)
    if B.ndim != 2:
        raise ValueError("b2rf_batch: B must be a (count, n) array")
    count, n = B.shape
    if count < 1 or not 2 <= n <= 2048:
        raise ValueError("b2rf_batch: need count >= 1 and 2 <= n <= 2048 (got %d x %d)" % (count, n))
    ctx = ctx or get_context()
    bre, bim = np.ascontiguousarray(B.real), np.ascontiguousarray(B.imag)
    rre, rim = np.zeros((count, n)), np.zeros((count, n))
    rc = load_library().mbfir_b2rf_batch(ctx._h, n, count, _ptr(bre), _ptr(bim), _ptr(rre), _ptr(rim))
    if rc == E_ARG:
        raise ValueError("b2rf_batch: %s" % ctx.last_error())
    _check(ctx, rc)
    return rre + 1j * rim


def slr2d_batch(R, *, literal=False, ctx=None):
    """The 2D inverse SLR of dzepse.m:39-49 for every matrix of a (count, m, n) complex array in one call (mbfir_slr2d_batch):
    rows are spatial samples, columns spectral samples; 2 <= n <= 2048, 2 <= m <= 2048, m even.  Returns rn2 (count, m, n) in
    radians per sample.  The middle stage takes the hard-pulse beta sin(|theta| / 2) exp(-i arg theta) of every stage-1 angle,
    which is dzepse's sin(conj(theta) / 2) for a real theta; literal=True takes dzepse's form itself (its own stage-1 angles are
    not real).  A matrix's result does not depend on the rest of the batch."""
    R = np.asarray(R, dtype=np.complex128)
    if R.ndim != 3:
        raise ValueError("slr2d_batch: R must be a (count, m, n) array")
    count, m, n = R.shape
    if count < 1 or not 2 <= n <= 2048 or not 2 <= m <= 2048 or m % 2:
        raise ValueError("slr2d_batch: need count >= 1, 2 <= n <= 2048 and an even 2 <= m <= 2048 (got %d x %d x %d)"
                         % (count, m, n))
    ctx = ctx or get_context()
    rre, rim = np.ascontiguousarray(R.real), np.ascontiguousarray(R.imag)
    ore, oim = np.zeros((count, m, n)), np.zeros((count, m, n))
    rc = load_library().mbfir_slr2d_batch(ctx._h, m, n, count, _ptr(rre), _ptr(rim), _ptr(ore), _ptr(oim),
                                                  int(bool(literal)))
    if rc == E_ARG:
        raise ValueError("slr2d_batch: %s" % ctx.last_error())
    _check(ctx, rc)
    return ore + 1j * oim


def _pack_masks(masks):
    """nz x ncand 0/1 matrix (a column per candidate, fir_flip_zero's layout) -> ncand x ceil(nz / 32) uint32 words, bit j = row j."""
    m = np.asarray(masks).astype(bool)
    nz, num = m.shape
    words = (nz + 31) // 32
    pad = np.zeros((words * 32, num), dtype=np.uint64)
    pad[:nz] = m
    w = (pad.reshape(words, 32, num) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1)
    return np.ascontiguousarray(w.T.astype(np.uint32))


def flip_search(c0, z, zf, *, masks=None, enum_bits=None, ncand=None, target=None, bsf=None, criterion="beta", tie_high=False,
                return_peaks=False, ctx=None):
    """Root-flip search on the device (mbfir_flip_search): candidate = poly c0 times prod_j (x - z_j or x - zf_j), scaled to
    sum(beta) = target (fir_flip_zero.m:83) or npoly-normalised times bsf (minpeakrf.c), scored by its largest |beta_k|
    (criterion "beta") or its largest |rf_k| through b2rf (criterion "rf").  Candidates: `masks` (nz x ncand 0/1, a column per
    candidate, 1 = flipped), or all 2^nz in combination_2power order (fir_flip_zero.m:153-160), or, with `enum_bits` (nz ints) and
    `ncand`, c = 0 .. ncand-1 with factor j flipped iff bit (enum_bits[j] >> 1) of c equals enum_bits[j] & 1.
    Returns (winner's beta, winner's index, every candidate's peak or None)."""
    ctx = ctx or get_context()
    c0re, c0im = _split(c0)
    zre, zim = _split(z)
    fre, fim = _split(zf)
    nz = len(zre)
    if len(fre) != nz:
        raise ValueError("flip_search: z and zf must have the same length")
    n = len(c0re) + nz
    if (target is None) == (bsf is None):
        raise ValueError("flip_search: give exactly one of target (DC rule) and bsf (npoly rule)")
    if criterion not in ("beta", "rf"):
        raise ValueError("flip_search: criterion must be 'beta' or 'rf'")
    mk, eb = None, None
    if masks is not None:
        mk = _pack_masks(np.asarray(masks).reshape(nz, -1))
        ncand = mk.shape[0]
    elif enum_bits is not None:
        eb = np.ascontiguousarray(np.asarray(enum_bits, dtype=np.int32).ravel())
        if len(eb) != nz or ncand is None:
            raise ValueError("flip_search: enum_bits needs one entry per factor and ncand")
    else:
        if nz > 24:
            raise ValueError("flip_search: all 2^nz candidates only up to nz = 24 (got %d)" % nz)
        ncand = 2 ** nz
    ncand = int(ncand)
    pk = np.zeros(ncand) if return_peaks else None
    bre, bim = np.zeros(n), np.zeros(n)
    win, wp = C.c_long(-1), C.c_double(0)
    if target is not None:
        t = complex(target)
        rule, sre, sim = 0, t.real, t.imag
    else:
        rule, sre, sim = 1, float(bsf), 0.0
    rc = load_library().mbfir_flip_search(
        ctx._h, n, nz, _ptr(c0re), _ptr(c0im), _ptr(zre), _ptr(zim), _ptr(fre), _ptr(fim), ncand,
        mk.ctypes.data_as(C.POINTER(C.c_uint)) if mk is not None else None, eb.ctypes.data_as(_ip) if eb is not None else None,
        rule, sre, sim, 1 if criterion == "rf" else 0, 1 if tie_high else 0, _ptr(pk) if pk is not None else None,
        _ptr(bre), _ptr(bim), C.byref(win), C.byref(wp))
    if rc == E_ARG:
        raise ValueError("flip_search: arguments out of range (%s)" % ctx.last_error())
    if rc != 0:
        raise MbfirError("mbfir_flip_search failed (%d): %s" % (rc, ctx.last_error()))
    return bre + 1j * bim, int(win.value), pk


def test_flip_stages(c0, z, zf, *, masks=None, enum_bits=None, ncand=None, target=None, bsf=None, criterion="rf", tie_high=False,
                     force_mode=-1, max_blocks=0, sel=(), guard=0, fill=0.0, ctx=None):
    """Test hook (mbfir_test_flip_stages): flip_search under a forced kernel mode and a cap on the workgroups, then every stage of the
    candidates `sel` from one more launch.  Candidates and scale rule as flip_search (masks: nz x ncand).  Every output block is
    allocated `guard` elements longer than the hook may write and pre-filled with `fill`; "raw" holds those flat arrays whole, so a
    caller can see that nothing outside a block changed.  Returns a dict: status (0, or NUMERICAL when no candidate is finite), winner,
    winner_peak, beta (the pick launch's), peaks, blk_p / blk_i (the launched workgroups'), report (dict), and per selected candidate
    st_beta, st_bf, st_xl, st_xlfp, st_afa, st_a, st_theta, st_peak (with criterion "beta" only st_beta and st_peak are written)."""
    ctx = ctx or get_context()
    c0re, c0im = _split(c0)
    zre, zim = _split(z)
    fre, fim = _split(zf)
    nz = len(zre)
    n = len(c0re) + nz
    if (target is None) == (bsf is None):
        raise ValueError("test_flip_stages: give exactly one of target (DC rule) and bsf (npoly rule)")
    mk, eb = None, None
    if masks is not None:
        m = np.asarray(masks)
        ncand = m.shape[1] if m.ndim == 2 else m.size // max(nz, 1)
        mk = _pack_masks(m.reshape(nz, ncand))
    elif enum_bits is not None:
        eb = np.ascontiguousarray(np.asarray(enum_bits, dtype=np.int32).ravel())
    else:
        ncand = 2 ** nz
    ncand = int(ncand)
    sel = np.ascontiguousarray(np.asarray(sel, dtype=np.int64).ravel())
    ns = len(sel)
    sizes = dict(peaks=ncand, blk_p=ncand, beta_re=n, beta_im=n, st_beta=2 * ns * n, st_bf=ns * 8 * n, st_xl=ns * 8 * n,
                 st_xlfp=2 * ns * (4 * n + 1), st_afa=2 * ns * 8 * n, st_a=2 * ns * n, st_theta=ns * n, st_peak=ns)
    raw = {k: np.full(v + guard, fill, dtype=np.float64) for k, v in sizes.items()}
    raw["blk_i"] = np.full(ncand + guard, -7, dtype=np.int64)
    raw["report"] = np.full(8 + guard, -7, dtype=np.int64)
    win, wp = C.c_long(-7), C.c_double(0)
    if target is not None:
        t = complex(target)
        rule, sre, sim = 0, t.real, t.imag
    else:
        rule, sre, sim = 1, float(bsf), 0.0
    lp = lambda a: a.ctypes.data_as(_lp)                                            # noqa: E731
    rc = load_library().mbfir_test_flip_stages(
        ctx._h, n, nz, _ptr(c0re), _ptr(c0im), _ptr(zre), _ptr(zim), _ptr(fre), _ptr(fim), ncand,
        mk.ctypes.data_as(C.POINTER(C.c_uint)) if mk is not None else None, eb.ctypes.data_as(_ip) if eb is not None else None,
        rule, sre, sim, 1 if criterion == "rf" else 0, 1 if tie_high else 0, int(force_mode), int(max_blocks), ns, lp(sel),
        _ptr(raw["peaks"]), _ptr(raw["blk_p"]), lp(raw["blk_i"]), _ptr(raw["beta_re"]), _ptr(raw["beta_im"]), C.byref(win), C.byref(wp),
        *[_ptr(raw[k]) for k in ("st_beta", "st_bf", "st_xl", "st_xlfp", "st_afa", "st_a", "st_theta", "st_peak")], lp(raw["report"]))
    if rc == E_ARG:
        raise ValueError("test_flip_stages: %s" % ctx.last_error())
    if rc not in (0, NUMERICAL):
        raise MbfirError("mbfir_test_flip_stages failed (%d): %s" % (rc, ctx.last_error()))
    rep = dict(zip(("mode", "threads", "blocks", "lds", "stride", "lds_limit", "nn", "words"), (int(v) for v in raw["report"][:8])))
    cplx = lambda k, m: (raw[k][:2 * ns * m:2] + 1j * raw[k][1:2 * ns * m:2]).reshape(ns, m)   # noqa: E731
    real = lambda k, m: raw[k][:ns * m].reshape(ns, m).copy()                       # noqa: E731
    nb = rep["blocks"]
    return dict(status=rc, winner=int(win.value), winner_peak=float(wp.value), beta=raw["beta_re"][:n] + 1j * raw["beta_im"][:n],
                peaks=raw["peaks"][:ncand].copy(), blk_p=raw["blk_p"][:nb].copy(), blk_i=raw["blk_i"][:nb].copy(), report=rep,
                st_beta=cplx("st_beta", n), st_bf=real("st_bf", 8 * n), st_xl=real("st_xl", 8 * n), st_xlfp=cplx("st_xlfp", 4 * n + 1),
                st_afa=cplx("st_afa", 8 * n), st_a=cplx("st_a", n), st_theta=real("st_theta", n), st_peak=raw["st_peak"][:ns].copy(),
                raw=raw, sizes=sizes)


def _flip_root(z):
    return z / (z.real ** 2 + z.imag ** 2)                # minpeakrf.c flip_root


def minpeakrf(z, flip, bsf, *, ctx=None):
    """`zmin = minpeakrf(z, flip, bsf)` (rf_tools/mex5/minpeakrf.c): of every combination of root flips, the roots whose beta
    polynomial (npoly-normalised, times bsf) gives the smallest RF peak.  flip: nflip x 2 matrix of 1-based root indices, second
    column 0 = a single root, otherwise a conjugate pair (bit 0 flips the second root, bit 1 the first; a pair on opposite sides of
    the unit circle has its first root flipped before the search).  Singles take the low bits of the combination index, pairs the
    next ones; the running minimum starts at the peak of the unflipped roots with index 0 and a candidate replaces it when its
    peak is <= the minimum.  Scored on the device through this package's b2rf (b2a.m's 8 n padding), not b2a.code.c's.
    Exhaustive up to 24 flip units (2^24 combinations)."""
    z = np.asarray(z, dtype=np.complex128).ravel()
    nroots = len(z)
    if nroots + 1 > 1024:
        raise ValueError("minpeakrf: z vector too long")
    bsf = float(np.asarray(bsf).ravel()[0])
    if not (0.0 <= bsf <= 1.0):
        raise ValueError("minpeakrf: bsf not in 0..1")
    fl = np.asarray(flip, dtype=np.float64)
    if fl.size == 0:
        fl = np.zeros((0, 2))
    if fl.ndim != 2 or fl.shape[1] != 2:
        raise ValueError("minpeakrf: flip must be an nflip x 2 matrix")
    if np.any(fl != np.round(fl)) or np.any(fl[:, 0] < 1) or np.any(fl > nroots) or np.any(fl[:, 1] < 0):
        raise ValueError("minpeakrf: bad root index in flip")
    fl = fl.astype(np.int64)
    singles = [int(r[0]) - 1 for r in fl if r[1] == 0]
    pairs = [(int(r[0]) - 1, int(r[1]) - 1) for r in fl if r[1] != 0]
    used = singles + [r for p in pairs for r in p]
    if len(set(used)) != len(used):
        raise ValueError("minpeakrf: a root is listed more than once in flip")
    nflip = len(singles) + len(pairs)
    if nflip > 24:
        raise ValueError("minpeakrf: more than 24 flip units (2^24 combinations)")
    z0 = z.copy()
    for r1, r2 in pairs:                                    # same side of the unit circle first
        if (abs(z[r1]) - 1) / (abs(z[r2]) - 1) < 0:
            z0[r1] = _flip_root(z[r1])
    fac, bits = [], []
    for u, r in enumerate(singles):
        fac.append(r)
        bits.append((u << 1) | 1)
    for u, (r1, r2) in enumerate(pairs, start=len(singles)):
        fac += [r1, r2]
        bits += [(u << 1) | 1, (u << 1) | 0]               # bit 1 flips the first, bit 0 the second
    fixed = np.ones(nroots, dtype=bool)
    fixed[fac] = False
    from .flipzero import _poly
    c0 = _poly(z0[fixed])
    zr = z0[fac]
    _, _, p0 = flip_search(_poly(z0), [], [], bsf=bsf, criterion="rf", return_peaks=True, ctx=ctx)
    _, best, pk = flip_search(c0, zr, _flip_root(zr), enum_bits=bits, ncand=2 ** nflip, bsf=bsf, criterion="rf", tie_high=True,
                              return_peaks=True, ctx=ctx)
    idx = best if pk[best] <= p0[0] else 0
    zmin = z0.copy()
    for j, r in enumerate(fac):
        if ((idx >> (bits[j] >> 1)) & 1) == (bits[j] & 1):
            zmin[r] = _flip_root(z0[r])
    return zmin


def abrm(rf, g=None, x=None, y=None, *, hard_pulse=False, ctx=None):
    """`[a b] = abrm(rf, g, x)` (rf_tools/abrm.m): Cayley-Klein parameters of the pulse at positions x; with two
    arguments the second one is x.  hard_pulse=True simulates the model ab2rf inverts exactly instead.
    `[a b] = abrm(rf, g, x, y)` (abrm.m:39-57): a 2D pulse, g complex (Re g the x gradient, Im g the y one), a and b of shape
    (len(x), len(y)) (mbfir_abr2; abrm's joint rotation only)."""
    ctx = ctx or get_context()
    if y is not None:
        if x is None or hard_pulse:
            raise ValueError("abrm: the 2D form takes rf, g, x, y (and no hard_pulse)")
        return _abrm2(rf, g, x, y, ctx)
    if x is None:
        x, g = g, None
    rre, rim = _split(rf)
    xv = _vec(x)
    gv = _vec(g) if g is not None else None
    if gv is not None and len(gv) != len(rre):
        raise ValueError("abrm: g must have one entry per rf sample")
    out = [np.zeros(len(xv)) for _ in range(4)]
    _check(ctx, load_library().mbfir_abr(ctx._h, len(rre), _ptr(rre), _ptr(rim), _ptr(gv) if gv is not None else None,
                                         len(xv), _ptr(xv), 1 if hard_pulse else 0, *[_ptr(o) for o in out]))
    return out[0] + 1j * out[1], out[2] + 1j * out[3]


def _abrm2(rf, g, x, y, ctx):
    rre, rim = _split(rf)
    xv, yv = _vec(x), _vec(y)
    if g is None:
        gx = gy = None
    else:
        gre, gim = _split(g)
        if len(gre) != len(rre):
            raise ValueError("abrm: g must have one entry per rf sample")
        gx, gy = gre, gim
    if len(xv) < 1 or len(yv) < 1:
        raise ValueError("abrm: x and y must not be empty")
    out = [np.zeros((len(xv), len(yv))) for _ in range(4)]
    rc = load_library().mbfir_abr2(ctx._h, len(rre), _ptr(rre), _ptr(rim), _ptr(gx) if gx is not None else None,
                                   _ptr(gy) if gy is not None else None, len(xv), _ptr(xv), len(yv), _ptr(yv),
                                   *[_ptr(o) for o in out])
    if rc == E_ARG:
        raise ValueError("abrm: %s" % ctx.last_error())
    _check(ctx, rc)
    return out[0] + 1j * out[1], out[2] + 1j * out[3]


def abr(rf, g=None, x=None, y=None, *, ctx=None):
    """`[a b] = abr(rf, g, x[, y])` (rf_tools/abr.m:19-34): abrm with Le Roux's convention on beta, b = -conj(b)."""
    a, b = abrm(rf, g, x, y, ctx=ctx)
    return a, -np.conj(b)


def rfscaleg(rf, t, gamma):
    """`rfs = rfscaleg(rf, t, gamma)` (rfscaleg.m:12-16): radians -> Gauss; t in ms, gamma in kHz/G."""
    rf = np.asarray(rf)
    return rf / (2 * np.pi * gamma * (t / len(rf)))


from . import spec          # noqa: E402  (physical multiband description -> (f, a, d); host only)
from . import io            # noqa: E402  (rfwrite / rfwrite_varian / signa)
from .io import rfwrite, rfwrite_varian, signa   # noqa: E402
from .flipzero import fir_flip_zero   # noqa: E402  (fir_flip_zero.m; its device search: flip_search above)
from .dzrf import dzrf_mb, fir_upsample, rf_mrange_desired   # noqa: E402  (dzrf_mb.m driver)
from .search import fir_ap, fir_qp, fir_min_order_linprog, fir_min_order_qprog_phs   # noqa: E402  (outer bisections)
from . import slrclassic    # noqa: E402  (conventional SLR pulses, dzrf.m and its designers; device remez and fmp)
from .slrclassic import (remez, remez_batch, fmp, msinc, firls_lp, dzlp, dzls, dzmp, dzrf_batch,   # noqa: E402
                         sim_rf_scale, sim_rf_scale_batch)
from . import epse          # noqa: E402  (dzepse.m spectral-spatial pulses and its helpers; device b2rf_batch)
from .epse import (fftc, fftcp, dzbeta, verse, versec, ab2ex, ab2se, ab2inv, ab2sat, ab2st, dzepse,   # noqa: E402
                   dzepse_batch)
from . import spiral        # noqa: E402  (dz2d.m / csg.m spiral 2D pulses and the k-space helpers; host only)
from .spiral import csg, dz2d, dz2d_batch, ktog, ktos, gt2cm   # noqa: E402
from . import ssmb          # noqa: E402  (multiband spectral-spatial pulses: dzrf_mb's spectral beta, device 2D SLR)
from .ssmb import dzss_mb, dzss_mb_batch, fold_bands   # noqa: E402
from . import torchsim      # noqa: E402  (torch.autograd wrappers of abr_batch / abr2_batch / bloch_batch; torch is imported on first use)
# `mbfir.dzrf` becomes the conventional designer (dzrf.m).  The module of dzrf_mb stays importable as `mbfir.dzrf` through
# sys.modules (`from mbfir.dzrf import dzrf_mb`), and the function carries that module's public names for attribute access.
dzrf = slrclassic.dzrf
for _n in ("dzrf_mb", "fir_upsample", "rf_mrange_desired"):
    setattr(dzrf, _n, globals()[_n])
del _n

_WHICH = {"fir_ap_cvx": 0, "fir_qp_cvx": 1, "fir_linprog": 2, "fir_qprog_phs": 3}
_pools = {}


def get_pool(streams=4, device=None):
    """`streams` contexts (one HIP stream each) on one device, created once and reused."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    key = (device, streams)
    if key not in _pools:
        _pools[key] = [Context(device) for _ in range(streams)]
    return _pools[key]


def _pack_jobs(jobs, solutions=False):
    """(designer, args) pairs as an array of struct mbfir_job; `keep` holds the arrays the structs point into."""
    arr = (Job * len(jobs))()
    keep = []
    for q, (name, args) in enumerate(jobs):
        which = _WHICH[name]
        n, f = int(args[0]), _vec(args[1])
        params = [0.0] * 4
        if which == 3:
            ac = np.asarray(args[2], dtype=np.complex128).ravel()
            dc = np.asarray(args[3], dtype=np.complex128).ravel()
            if len(f) % 2 or len(ac) != len(f) or len(dc) != len(f) // 2:
                raise ValueError("f, ac, dc have inconsistent lengths")
            a, d = _vec(np.stack([ac.real, ac.imag], 1)), _vec(np.stack([dc.real, dc.imag], 1))
            nband = len(dc)
        else:
            a, d = _vec(args[2]), _vec(args[3])
            _check_spec(f, a, d)
            nband = len(d)
            if which == 0:
                params[0] = float(args[4]) if len(args) > 4 else 0.0
                params[1] = float(args[5]) if len(args) > 5 else 1e-3
            elif which == 1:
                params[0] = float(args[4]) if len(args) > 4 else 100.0
                objv = _vec(args[5] if len(args) > 5 else 0.0)
                if len(objv) not in (1, 2):
                    raise ValueError("invalid input of obj")
                params[1:1 + len(objv)] = list(objv)
                params[3] = float(len(objv))
        hre, him = np.zeros(n), np.zeros(n)
        zbuf = np.zeros(4 * n + 16) if solutions else None       # every designer has at most 2n + 3 unknowns; checked below
        keep.append((f, a, d, hre, him, zbuf))
        J = arr[q]
        if solutions:
            J.z, J.z_cap = _ptr(zbuf), len(zbuf)
        J.which, J.n, J.nband = which, n, nband
        J.f, J.a, J.d, J.h_re, J.h_im = _ptr(f), _ptr(a), _ptr(d), _ptr(hre), _ptr(him)
        for t in range(4):
            J.params[t] = params[t]
    return arr, keep


def solve_batch(jobs, *, opts=None, streams=4, ctxs=None, info=False, solutions=False):
    """Independent designs, `streams` in flight at a time on one GPU (mbfir_solve_batch): the shape of
    the reference's outer loops -- the probes of a min-order / min-duration bisection, parameter sweeps.
    jobs: sequence of (designer, args) with designer in {'fir_ap_cvx', 'fir_qp_cvx', 'fir_linprog',
    'fir_qprog_phs'} and args the positional arguments of that function (n, f, a, d, ...).
    Returns a list of (h, status) -- or (h, status, info) -- in job order, as the single calls return.
    solutions=True appends the conic solution z of every job (mbfir_last_solution) to its tuple."""
    ctxs = ctxs or get_pool(streams)
    o = opts if opts is not None else make_opts()
    arr, keep = _pack_jobs(jobs, solutions)
    handles = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    load_library().mbfir_solve_batch(handles, len(ctxs), arr, len(jobs), C.byref(o))
    out = []
    for q in range(len(jobs)):
        hre, him = keep[q][3], keep[q][4]
        inf = Info.from_buffer_copy(arr[q].info)
        # errors are reported per job, like the single calls do (which context ran it is not recorded)
        if arr[q].rc < 0:
            if arr[q].rc == E_ARG:
                raise ValueError("job %d: invalid argument" % q)
            raise MbfirError("job %d failed (%d): %s" % (q, arr[q].rc, arr[q].err.decode(errors="replace")))
        res = _finish(ctxs[0], arr[q].rc, hre, him, inf, info)
        if solutions and inf.n_unknowns > len(keep[q][5]):
            raise MbfirError("job %d: the conic solution has %d unknowns, the buffer %d" % (q, inf.n_unknowns, len(keep[q][5])))
        out.append(res + (keep[q][5][: inf.n_unknowns],) if solutions else res)
    return out


def _check_spec(f, a, d):
    if len(f) % 2 or len(a) != len(f) or len(d) != len(f) // 2:
        raise ValueError("f, a, d have inconsistent lengths")


# ---- host-only introspection (no GPU): structured program -> dense (c, G, h) -------------------
def assemble_dense(which, n, f, a, d, params=(0.0,), grid_m=0, shard=None, rows=None):
    """Run the product's C++ problem assembly for designer `which` (0 ap, 1 qp, 2 linprog,
    3 qprog_phs; for 3 pass complex a, d) and expand the structured rows to dense arrays.
    shard=(rank, size) returns the rows that rank keeps in a row-sharded solve.
    rows: expand only these rows of G / h (a program too large to expand whole, e.g. n=2048, m=131072).
    Returns (rc, dict) -- used by the CPU tests to compare against the oracle."""
    lib = load_library()
    f = _vec(f)
    if which == 3:
        ac = np.asarray(a, dtype=np.complex128).ravel()
        dc = np.asarray(d, dtype=np.complex128).ravel()
        a = _vec(np.stack([ac.real, ac.imag], 1))
        d = _vec(np.stack([dc.real, dc.imag], 1))
    else:
        a, d = _vec(a), _vec(d)
    params = _vec(list(params) + [0.0] * 4)
    out = C.c_void_p()
    err = C.create_string_buffer(256)
    rc = lib.mbfir_assemble(which, int(n), len(f) // 2, _ptr(f), _ptr(a), _ptr(d), _ptr(params), int(grid_m),
                            C.byref(out), err, 256)
    if rc != 0:
        return rc, err.value.decode()
    if shard is not None:
        sub = C.c_void_p()
        rc2 = lib.mbfir_program_shard(out, int(shard[0]), int(shard[1]), C.byref(sub))
        lib.mbfir_program_free(out)
        if rc2 != 0:
            return rc2, "bad shard"
        out = sub
    try:
        dims = np.zeros(10, dtype=np.int32)
        lib.mbfir_program_dims(out, dims.ctypes.data_as(_ip))
        Nt, Ne, R, l, nq3, big, Mf, quad = [int(v) for v in dims[:8]]
        w = np.zeros(Mf)
        kind = np.zeros(Nt, dtype=np.int32)
        tau, scale, psign = np.zeros(Nt), np.zeros(Nt), np.zeros(Nt)
        pcol = np.zeros(Nt, dtype=np.int32)
        c = np.zeros(Nt + Ne)
        lib.mbfir_program_trig(out, _ptr(w), kind.ctypes.data_as(_ip), _ptr(tau), _ptr(scale),
                               pcol.ctypes.data_as(_ip), _ptr(psign), _ptr(c))
        freq = np.zeros(R, dtype=np.int32)
        col = np.zeros(R, dtype=np.int32)
        al, be, ey, h = np.zeros(R), np.zeros(R), np.zeros((R, 3)), np.zeros(R)
        lib.mbfir_program_rows(out, freq.ctypes.data_as(_ip), col.ctypes.data_as(_ip), _ptr(al), _ptr(be),
                               _ptr(ey), _ptr(h))
        rep = np.zeros(R, dtype=np.int32)
        lib.mbfir_program_replicated(out, rep.ctypes.data_as(_ip))
    finally:
        lib.mbfir_program_free(out)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        freq, col, al, be, ey, h, rep = freq[rows], col[rows], al[rows], be[rows], ey[rows], h[rows], rep[rows]
        used, inv = np.unique(freq[freq >= 0], return_inverse=True)
        wsub = w[used]
        fmap = np.full(len(freq), -1, dtype=np.int64)
        fmap[freq >= 0] = inv
    else:
        wsub, fmap = w, freq
    arg = np.outer(wsub, tau)
    A1 = scale * np.where(kind == 0, np.cos(arg), np.sin(arg))
    A2 = psign * A1[:, pcol] if quad else np.zeros_like(A1)
    G = np.zeros((len(freq), Nt + Ne))
    tr = fmap >= 0
    G[tr, :Nt] = al[tr, None] * A1[fmap[tr]] + be[tr, None] * A2[fmap[tr]]
    idr = np.nonzero(col >= 0)[0]
    G[idr, col[idr]] += al[idr]
    G[:, Nt:] = ey[:, :Ne]
    return 0, dict(c=c, G=G, h=h, l=l, nq3=nq3, big=big, w=w, Mf=Mf, Nt=Nt, Ne=Ne, quad=quad, freq=freq, R=R, rep=rep)


# ---- device kernel test hooks --------------------------------------------------------------------
def _check(ctx, rc):
    if rc != 0:
        raise MbfirError("mbfir test hook failed (%d): %s" % (rc, ctx.last_error()))


def test_gram(A, d, ctx=None):
    ctx = ctx or get_context()
    A = np.ascontiguousarray(A, dtype=np.float64)
    d = np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64)
    m, nt = A.shape
    nw = d.shape[0]
    out = np.zeros((nw, nt, nt))
    _check(ctx, load_library().mbfir_test_gram(ctx._h, m, nt, nw, _ptr(A), _ptr(d), _ptr(out)))
    return out


def test_chol(H, ctx=None):
    ctx = ctx or get_context()
    H = np.ascontiguousarray(H, dtype=np.float64)
    n = H.shape[0]
    L, M = np.zeros((n, n)), np.zeros((n, n))
    _check(ctx, load_library().mbfir_test_chol(ctx._h, n, _ptr(H), _ptr(L), _ptr(M)))
    return L, M


UNIT_OPS_REPORT = ("lattice", "pair_passes", "one_pass", "D1", "useg", "nfold", "nchunk", "cgrp", "np", "empty_side", "seg", "hetero",
                   "seeds_shared", "gv_passes", "gtv_passes", "lanes")


def test_unit_ops(jobs, v, u, s, z, *, sub=None, mask=None, opts=None, init=None, ctx=None):
    """The operators of one lock-step unit at the iterate (s, z) (mbfir_test_unit_ops).  jobs: (designer, args) pairs as for
    solve_batch, the lanes of the unit.  v: (lanes, nv, N) x-space vectors, u and sub: (lanes, nv, R) row-space vectors, s and z:
    (lanes, R); a lane shorter than the unit's largest is zero-padded by the caller.  init: the four output arrays (gv, gtu, wgv, H)
    as they go in (default NaN), so that what a masked lane returns can be compared with it.  Returns (gv, gtu, wgv, H, report):
    G v and W^-2 G v - sub (lanes, nv, R), G'u (lanes, nv, N), H (lanes, np, np; the lower triangle is meaningful), report a dict
    of UNIT_OPS_REPORT and tmin."""
    ctx = ctx or get_context()
    arr, keep = _pack_jobs(jobs)
    v, u = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    s, z = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(z, dtype=np.float64)
    nl, nv, N = v.shape
    R = u.shape[2]
    if nl != len(jobs) or u.shape != (nl, nv, R) or s.shape != (nl, R) or z.shape != (nl, R):
        raise ValueError("v, u, s, z have inconsistent shapes")
    npad = -(-N // 64) * 64
    if sub is not None:
        sub = np.ascontiguousarray(sub, dtype=np.float64)
        if sub.shape != u.shape:
            raise ValueError("sub must have the shape of u")
    if init is None:
        init = (np.full((nl, nv, R), np.nan), np.full((nl, nv, N), np.nan), np.full((nl, nv, R), np.nan), np.full((nl, npad, npad), np.nan))
    gv, gtu, wgv, H = [np.array(a, dtype=np.float64, order="C") for a in init]
    if gv.shape != u.shape or gtu.shape != v.shape or wgv.shape != u.shape or H.shape != (nl, npad, npad):
        raise ValueError("init arrays have the wrong shapes")
    mk = (C.c_int * nl)(*[int(m) for m in mask]) if mask is not None else None
    report = np.zeros(len(UNIT_OPS_REPORT), dtype=np.int64)
    tmin = np.zeros(1)
    o = opts if opts is not None else make_opts()
    rc = load_library().mbfir_test_unit_ops(ctx._h, arr, nl, C.byref(o), nv, N, R, npad, _ptr(v), _ptr(u),
                                            _ptr(sub) if sub is not None else None, _ptr(s), _ptr(z), mk, _ptr(gv), _ptr(gtu),
                                            _ptr(wgv), _ptr(H), report.ctypes.data_as(_lp), _ptr(tmin))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    rep = {k: int(x) for k, x in zip(UNIT_OPS_REPORT, report)}
    rep["tmin"] = float(tmin[0])
    return gv, gtu, wgv, H, rep


# the blocks of mbfir_test_unit_cone (include/mbfir.h): names of the rows of in_r / in_x / in_sc and out_r / out_x / out_sc
UNIT_CONE_IN_R = ("s", "z", "rz", "bz2a", "bz2b", "z1", "z2", "g1", "g2", "zc", "gc", "kz", "kg", "shift")
UNIT_CONE_IN_X = ("x", "rx", "x1", "x2", "xc", "kx")
UNIT_CONE_IN_SC = ("tau", "kappa", "mu", "rt", "sigmax", "dres", "nrmc", "rnc")
UNIT_CONE_OUT_R = ("dl", "wl", "lam", "wbz2a", "wbz2b", "wbb", "dssa", "wdza", "lds", "bzc", "wbzc", "ds", "dz", "kbz", "wbzk", "kzsum", "kgsum",
                   "kds", "kdz", "s", "z", "shift")
UNIT_CONE_OUT_X = ("bxc", "kxsum", "x")
UNIT_CONE_SNAPS = ("scaling", "pred", "comb_rhs", "comb", "corr_rhs", "update", "shift")
UNIT_CONE_SC = ("etab", "tau", "kappa", "sigma", "alpha", "alpha_a", "dtau", "dkap", "dtau_a", "dkap_a", "tmax", "tau0", "kap0", "alpha0",
                "dtau_c", "dkap_c", "pick", "ncorr", "npick", "wb0", "mu", "rb0", "rb1", "rb2")
UNIT_CONE_REPORT = ("cone_blocks", "l", "nq3", "big", "N", "R", "hetero", "lanes", "fuse", "corr_big", "form", "ns_affine", "ns_combined",
                    "update_blocks")


def test_unit_cone(jobs, in_r, in_x, in_sc, nq3, *, form=0, corrector=False, mask=None, opts=None, sentinel=np.nan, ctx=None):
    """The cone stages of one iteration of a lock-step unit at a caller's iterate (mbfir_test_unit_cone, which says what every
    block holds).  jobs: (designer, args) pairs, the lanes.  in_r: (lanes, 14, R), in_x: (lanes, 6, N), in_sc: (lanes, 8), rows
    named by UNIT_CONE_IN_*; a lane shorter than the unit's largest is zero-padded by the caller; nq3: the unit's largest count of
    3-row cones.  Every output block goes in
    filled with `sentinel`.  Returns a dict: out_r (lanes, 22, R), out_x (lanes, 3, N), w3 (lanes, max(nq3, 1), 4), sc (lanes, 7,
    24) -- rows named by UNIT_CONE_OUT_R / _OUT_X / _SNAPS x _SC -- and report (a dict of UNIT_CONE_REPORT)."""
    ctx = ctx or get_context()
    arr, keep = _pack_jobs(jobs)
    in_r, in_x, in_sc = [np.ascontiguousarray(a, dtype=np.float64) for a in (in_r, in_x, in_sc)]
    nl, R, N = len(jobs), in_r.shape[2], in_x.shape[2]
    if in_r.shape != (nl, len(UNIT_CONE_IN_R), R) or in_x.shape != (nl, len(UNIT_CONE_IN_X), N) or in_sc.shape != (nl, len(UNIT_CONE_IN_SC)):
        raise ValueError("in_r, in_x, in_sc have inconsistent shapes")
    lib = load_library()
    ldw = 4 * max(int(nq3), 1)
    out_r = np.full((nl, len(UNIT_CONE_OUT_R), R), sentinel)
    out_x = np.full((nl, len(UNIT_CONE_OUT_X), N), sentinel)
    w3 = np.full((nl, ldw // 4, 4), sentinel)
    sc = np.full((nl, len(UNIT_CONE_SNAPS), len(UNIT_CONE_SC)), sentinel)
    mk = (C.c_int * nl)(*[int(m) for m in mask]) if mask is not None else None
    report = np.zeros(16, dtype=np.int64)
    o = opts if opts is not None else make_opts()
    rc = lib.mbfir_test_unit_cone(ctx._h, arr, nl, C.byref(o), int(form), int(bool(corrector)), N, R, ldw, mk, _ptr(in_r), _ptr(in_x),
                                  _ptr(in_sc), _ptr(out_r), _ptr(out_x), _ptr(w3), _ptr(sc), report.ctypes.data_as(_lp))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return dict(out_r=out_r, out_x=out_x, w3=w3, sc=sc, report={k: int(x) for k, x in zip(UNIT_CONE_REPORT, report)})


# the blocks of mbfir_test_unit_kkt (include/mbfir.h)
UNIT_KKT_RES_R = ("rz", "bz2a", "bz2b")
UNIT_KKT_RES_X = ("gtz", "rx", "bx2a", "bx2b")
UNIT_KKT_RES_SC = ("rt", "mu", "pcost", "dcost", "gap", "relgap", "pres", "dres", "pinf", "dinf", "cx", "hz", "sz", "cholfix", "tau", "kappa",
                   "nrmh", "nrmc", "deg", "rb0", "rb1", "rb2", "rb3", "rb4")
UNIT_KKT_OUT_X = (("gtwbz", "dxc", "gtdz", "rc") + tuple("%s%d" % (k, q) for q in range(8) for k in ("p", "z")) +
                  tuple("%s%d" % (k, q) for q in range(8) for k in ("hp", "dx", "r")) + ("dx_end", "r_end"))
UNIT_KKT_OUT_R = (("wbz", "gdxc", "dzc") + tuple("%s%d" % (k, q) for q in range(8) for k in ("gp", "wp", "gdx", "dz")) + ("gdx_end", "dz_end"))
UNIT_KKT_SNAPS = ("resid",) + tuple("start%d" % q for q in range(8)) + tuple("step%d" % q for q in range(8)) + ("end",)
UNIT_KKT_SC = tuple("n%d" % q for q in range(9)) + ("rz0", "rz1", "alpha0", "alpha1")
UNIT_KKT_INIT_R = ("dl", "wl", "wbb", "s", "z", "bz2a", "bz2b")
UNIT_KKT_INIT_X = ("x", "bx2a", "bx2b")
UNIT_KKT_REPORT = ("fused_hsolve", "fuse", "form", "N", "R", "np", "big", "lanes", "hetero", "lattice", "gt_finish_blocks", "nv", "two",
                   "wbz_ready", "initial", "nsweep_max", "l", "nq3", "resid_blocks", "z_written", "gv_passes", "gtv_passes")


def test_unit_kkt(jobs, s, z, x, tau_kappa, nsweep, nq3, *, bx=None, bz=None, nv=2, initial=False, form=0, two=False, wbz_ready=False,
                  mask=None, opts=None, sentinel=np.nan, ctx=None):
    """The residual kernels and the plain KKT solve of a lock-step unit, group of launches by group (mbfir_test_unit_kkt, which says
    what every block holds).  jobs: (designer, args) pairs, the lanes.  s, z: (lanes, R); x: (lanes, N); tau_kappa: (lanes, 2);
    nsweep: the lanes' sweep counts; bx: (lanes, nv, N) and bz: (lanes, nv, R), or neither (nv = 2: the right-hand sides the
    residual kernels leave); nq3: the unit's largest count of 3-row cones.  Every output block goes in filled with `sentinel`.
    Returns a dict: res_r, res_x, res_sc, M (lanes, np, np), flag, out_x (lanes, 46, 2, N), out_r (lanes, 37, 2, R), sc (lanes, 18, 13),
    init_r, init_x, w3 (initial=True), rows named by UNIT_KKT_*, and report (a dict of UNIT_KKT_REPORT)."""
    ctx = ctx or get_context()
    arr, keep = _pack_jobs(jobs)
    s, z, x, tk = [np.ascontiguousarray(a, dtype=np.float64) for a in (s, z, x, tau_kappa)]
    nl, R, N = len(jobs), s.shape[1], x.shape[1]
    if s.shape != (nl, R) or z.shape != (nl, R) or x.shape != (nl, N) or tk.shape != (nl, 2) or len(nsweep) != nl:
        raise ValueError("s, z, x, tau_kappa, nsweep have inconsistent shapes")
    if (bx is None) != (bz is None):
        raise ValueError("bx and bz go together")
    if bx is not None:
        bx, bz = np.ascontiguousarray(bx, dtype=np.float64), np.ascontiguousarray(bz, dtype=np.float64)
        if bx.shape != (nl, nv, N) or bz.shape != (nl, nv, R):
            raise ValueError("bx, bz have the wrong shapes")
    npad = -(-N // 64) * 64
    ldw = 4 * max(int(nq3), 1)
    full = lambda *shape: np.full(shape, sentinel, dtype=np.float64)
    o = dict(res_r=full(nl, len(UNIT_KKT_RES_R), R), res_x=full(nl, len(UNIT_KKT_RES_X), N), res_sc=full(nl, len(UNIT_KKT_RES_SC)),
             M=full(nl, npad, npad), out_x=full(nl, len(UNIT_KKT_OUT_X), 2, N), out_r=full(nl, len(UNIT_KKT_OUT_R), 2, R),
             sc=full(nl, len(UNIT_KKT_SNAPS), len(UNIT_KKT_SC)), init_r=full(nl, len(UNIT_KKT_INIT_R), R),
             init_x=full(nl, len(UNIT_KKT_INIT_X), N), w3=full(nl, ldw // 4, 4))
    flag = np.full(nl, -1, dtype=np.int64)
    report = np.zeros(24, dtype=np.int64)
    mk = (C.c_int * nl)(*[int(m) for m in mask]) if mask is not None else None
    nsw = (C.c_int * nl)(*[int(q) for q in nsweep])
    op = opts if opts is not None else make_opts()
    rc = load_library().mbfir_test_unit_kkt(ctx._h, arr, nl, C.byref(op), int(bool(initial)), int(form), int(bool(two)), int(bool(wbz_ready)),
                                            int(nv), N, R, npad, ldw, mk, nsw, _ptr(s), _ptr(z), _ptr(x), _ptr(tk),
                                            _ptr(bx) if bx is not None else None, _ptr(bz) if bz is not None else None, _ptr(o["res_r"]),
                                            _ptr(o["res_x"]), _ptr(o["res_sc"]), _ptr(o["M"]), flag.ctypes.data_as(_lp), _ptr(o["out_x"]),
                                            _ptr(o["out_r"]), _ptr(o["sc"]), _ptr(o["init_r"]), _ptr(o["init_x"]), _ptr(o["w3"]),
                                            report.ctypes.data_as(_lp))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    o["flag"] = flag
    o["report"] = {k: int(v) for k, v in zip(UNIT_KKT_REPORT, report)}
    return o


# the blocks of mbfir_test_unit_ddkkt (include/mbfir.h)
UNIT_DDKKT_OUT_X = ("gtdz", "r1", "gtw", "rhs_h", "rhs_l", "y", "bh", "bl", "dx")
UNIT_DDKKT_OUT_R = ("r2", "wbz", "gbh", "wbz2", "dz", "gdx")
UNIT_DDKKT_OUT_K = ("ts", "capw", "zeta")
UNIT_DDKKT_REPORT = ("kp", "cap_form", "passes", "lanes", "N", "R", "np", "l", "nq3", "big", "k_max", "attempts", "nv", "solve", "hetero",
                     "nsweep_plain")
DD_KMAX = 3072


def test_unit_ddkkt(jobs, s, z, bx, bz, nq3, *, solve=True, ldu=64, cap_blocks=True, mask=None, opts=None, sentinel=np.nan, ctx=None):
    """The extended-precision path of an iteration of a lock-step unit, stage by stage (mbfir_test_unit_ddkkt, which says what every
    block holds).  jobs: (designer, args) pairs, the lanes.  s, z: (lanes, R); bx: (lanes, nv, N); bz: (lanes, nv, R); nq3: the unit's
    largest count of 3-row cones; ldu: the rows of U (and of Yt, Zt, S, Ms with cap_blocks) to return.  Every output block goes in
    filled with `sentinel` (the integer blocks with -9).  Returns a dict of the blocks, rows named by UNIT_DDKKT_*, with lane_rep
    (lanes, 4) and report (a dict of UNIT_DDKKT_REPORT)."""
    ctx = ctx or get_context()
    arr, keep = _pack_jobs(jobs)
    s, z, bx, bz = [np.ascontiguousarray(a, dtype=np.float64) for a in (s, z, bx, bz)]
    nl, R = len(jobs), s.shape[1]
    if bx.ndim != 3 or bz.ndim != 3:
        raise ValueError("bx, bz: (lanes, nv, N) and (lanes, nv, R)")
    nv, N = bx.shape[1], bx.shape[2]
    if s.shape != (nl, R) or z.shape != (nl, R) or bx.shape != (nl, nv, N) or bz.shape != (nl, nv, R):
        raise ValueError("s, z, bx, bz have inconsistent shapes")
    npad = -(-N // 64) * 64
    # (the blocks of unknowns are np wide: the capacitance form's vectors are, and what lies past N shows there)
    bx, N = np.concatenate([bx, np.zeros((nl, nv, npad - N))], axis=2), npad
    nq = max(int(nq3), 1)
    ldu = int(ldu)
    full = lambda *shape: np.full(shape, sentinel, dtype=np.float64)
    ints = lambda *shape: np.full(shape, -9, dtype=np.int32)
    ldp = -(-R // 256) + 2
    o = dict(sel_r=full(nl, 4, R), sel_q=full(nl, 18 * nq), sel_sc=full(nl, 16), sel_part=full(nl, ldp, 2), sel_i=ints(nl, R + 3 * nq + 3), strong_i=ints(nl, 3, DD_KMAX),
             strong_x=full(nl, DD_KMAX), H=full(nl, npad, npad), U=full(nl, ldu, npad), M=full(nl, npad, npad), Hf=full(nl, npad, npad),
             out_x=full(nl, 3, len(UNIT_DDKKT_OUT_X), 2, N), out_r=full(nl, 3, len(UNIT_DDKKT_OUT_R), 2, R),
             out_k=full(nl, 3, len(UNIT_DDKKT_OUT_K), 2, DD_KMAX), sc=full(nl, 4, 9), end_x=full(nl, 2, N), end_r=full(nl, 2, 2, R))
    if cap_blocks:
        o.update(Yt=full(nl, ldu, npad), Zt=full(nl, ldu, npad), S=full(nl, ldu, ldu), Ms=full(nl, ldu, ldu))
    flag = np.full(nl, -1, dtype=np.int64)
    lane_rep, report = np.zeros((nl, 4), dtype=np.int64), np.zeros(16, dtype=np.int64)
    mk = (C.c_int * nl)(*[int(m) for m in mask]) if mask is not None else None
    op = opts if opts is not None else make_opts(ddkkt=1)
    ipt = lambda a: a.ctypes.data_as(_ip)
    cb = lambda k: _ptr(o[k]) if cap_blocks else None
    rc = load_library().mbfir_test_unit_ddkkt(ctx._h, arr, nl, C.byref(op), int(nv), int(bool(solve)), N, R, npad, 4 * nq, ldu, ldp, mk, _ptr(s), _ptr(z),
                                              _ptr(bx), _ptr(bz), _ptr(o["sel_r"]), _ptr(o["sel_q"]), _ptr(o["sel_sc"]), _ptr(o["sel_part"]), ipt(o["sel_i"]),
                                              ipt(o["strong_i"]), _ptr(o["strong_x"]), _ptr(o["H"]), _ptr(o["U"]), _ptr(o["M"]), _ptr(o["Hf"]),
                                              cb("Yt"), cb("Zt"), cb("S"), cb("Ms"), flag.ctypes.data_as(_lp), _ptr(o["out_x"]), _ptr(o["out_r"]),
                                              _ptr(o["out_k"]), _ptr(o["sc"]), _ptr(o["end_x"]), _ptr(o["end_r"]), lane_rep.ctypes.data_as(_lp),
                                              report.ctypes.data_as(_lp))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    o["flag"], o["lane_rep"] = flag, lane_rep
    o["report"] = {k: int(v) for k, v in zip(UNIT_DDKKT_REPORT, report)}
    return o


def test_chol_lanes(Hs, form=-1, mask=None, ctx=None):
    """Hs: (nlanes, n, n) SPD matrices factorised together like a lock-step batch; returns (L, M) of shape (nlanes, n, n)."""
    ctx = ctx or get_context()
    Hs = np.ascontiguousarray(Hs, dtype=np.float64)
    nl, n = Hs.shape[0], Hs.shape[1]
    L, M = np.zeros((nl, n, n)), np.zeros((nl, n, n))
    mk = None
    if mask is not None:
        mk = (C.c_int * nl)(*[int(v) for v in mask])
    _check(ctx, load_library().mbfir_test_chol_lanes(ctx._h, n, nl, int(form), mk, _ptr(Hs), _ptr(L), _ptr(M)))
    return L, M


GAMMA_C13 = 6726.1          # rad/s/G, blochC.c:5
GAMMA_H1 = 26754.0          # blochH.c:6


def _bloch_pulse(b1, gr, tp, nucleus):
    """One pulse as bloch takes it -> b1 (ntime,), gr (ntime, axes), tp as one interval or ntime intervals, gamma."""
    b1 = np.asarray(b1, dtype=np.complex128).ravel()
    nt = len(b1)
    gr = np.zeros((nt, 1)) if gr is None else np.asarray(gr, dtype=np.float64).reshape(nt, -1)
    tp = np.asarray(tp, dtype=np.float64).ravel()
    if tp.size != 1 and tp.size != nt:
        raise MbfirError("Time-point length differs from B1 length")
    if tp.size > 1:
        iv = np.diff(np.concatenate([[0.0], tp]))
        tp = iv if np.all(iv > 0) else tp                       # increasing end times -> intervals (times2intervals)
    return b1, gr, tp, GAMMA_C13 if nucleus == "C-13" else GAMMA_H1 if nucleus == "H-1" else float(nucleus)


def bloch(b1, gr, tp, t1, t2, df, dp, mode=0, mx=None, my=None, mz=None, nucleus="C-13", ctx=None):
    """[mx, my, mz] = bloch(b1, gr, tp, t1, t2, df, dp, mode, mx, my, mz) of bloch_simulation/bloch.m:1-44 on the device
    (blochC for nucleus 'C-13', blochH for 'H-1', as sim_rf_spectral.m:53-60 picks them).  b1 complex (Gauss), gr (ntime,)
    or (ntime, 1..3) G/cm, tp a scalar interval, ntime intervals, or ntime monotonically increasing end times
    (blochC.c:649-681), df Hz, dp (npos,) or (npos, 1..3) cm.  Returns arrays of shape (nfreq, npos) or, with mode & 2,
    (nfreq, npos, ntime)."""
    ctx = ctx or get_context()
    b1, gr, tp, gamma = _bloch_pulse(b1, gr, tp, nucleus)
    nt = len(b1)
    g3 = [_vec(gr[:, i]) if i < gr.shape[1] else None for i in range(3)]
    ts = np.full(nt, tp[0]) if tp.size == 1 else tp
    df = _vec(df)
    dp = np.asarray(dp, dtype=np.float64)
    dp = dp.reshape(-1, 1) if dp.ndim < 2 else dp
    p3 = [_vec(dp[:, i]) if i < dp.shape[1] else None for i in range(3)]
    nf, npos = len(df), dp.shape[0]
    ntout = nt if (int(mode) & 2) else 1
    out = []
    for init, dflt in ((mx, 0.0), (my, 0.0), (mz, 1.0)):
        o = np.zeros((nf * npos, ntout))
        o[:, 0] = dflt if init is None or np.size(init) != nf * npos else np.asarray(init, dtype=np.float64).ravel()
        out.append(np.ascontiguousarray(o))
    nul = C.cast(None, _dp)
    _check(ctx, load_library().mbfir_bloch(ctx._h, nt, _ptr(_vec(b1.real)), _ptr(_vec(b1.imag)),
                                           *[_ptr(g) if g is not None else nul for g in g3], _ptr(_vec(ts)), float(t1), float(t2),
                                           nf, _ptr(df), npos, *[_ptr(p) if p is not None else nul for p in p3], int(mode),
                                           gamma, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
    shape = (nf, npos, nt) if ntout > 1 else (nf, npos)
    return tuple(o.reshape(shape) for o in out)


# ---- batched simulators: many pulses x transmit-gain scales in one launch (mbfir_bloch_batch, mbfir_abr[2]_batch) -------------
def _offsets(lengths):
    """offset table of a concatenated list (C long): 0, then the running sums"""
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64))


def _lptr(a):
    return a.ctypes.data_as(_lp)


def _per_pulse(v, npulse):
    """A Python list of npulse arrays is one grid per pulse; anything else is one grid shared by every pulse."""
    if isinstance(v, list) and len(v) == npulse and all(np.ndim(e) >= 1 for e in v):
        return list(v)
    return [v]


def sim_block_table(ntime, npoint, nscale):
    """The workgroups of bloch_batch / abr_batch in launch order (host only, mbfir_test_sim_blocks): one row (pulse, scale, chunk)
    per 256-thread workgroup for pulses of ntime[p] samples and npoint[p] points at nscale scales, the longest pulses first."""
    nt = np.ascontiguousarray(ntime, dtype=np.int32)
    npt = np.ascontiguousarray(npoint, dtype=np.int64)
    if len(nt) != len(npt):
        raise ValueError("sim_block_table: ntime and npoint differ in length")
    lib = load_library()
    k = lib.mbfir_test_sim_blocks(len(nt), nt.ctypes.data_as(_ip), _lptr(npt), int(nscale), None)
    if k < 0:
        raise ValueError("sim_block_table: need pulses, nscale >= 1, every ntime and npoint >= 1")
    out = np.zeros((k, 4), dtype=np.int32)
    lib.mbfir_test_sim_blocks(len(nt), nt.ctypes.data_as(_ip), _lptr(npt), int(nscale), out.ctypes.data_as(_ip))
    return out[:, :3]


class _BlochArgs:
    """The checked arguments of bloch_batch, bloch_vjp_batch and bloch_jvp_batch: the scales, the per-pulse sizes nt / nf / npos, and `head`, the
    arguments of the C calls from npulse up to and including scales (the arrays they point to are kept in `keep`)."""

    def __init__(self, who, pulses, df, dp, scales):
        pulses, sc = list(pulses), _vec(scales)
        if not pulses:
            raise ValueError("%s: no pulses" % who)
        if len(sc) == 0:
            raise ValueError("%s: the scale list is empty" % who)
        P = len(pulses)
        b1s, grs, tss, t1s, t2s, gams = [], [], [], [], [], []
        for q, (b1, gr, tp, t1, t2, nucleus) in enumerate(pulses):
            if np.size(b1) == 0:
                raise ValueError("%s: pulse %d has no samples" % (who, q))
            b1, gr, tp, gamma = _bloch_pulse(b1, gr, tp, nucleus)
            if gr.shape[1] > 3:
                raise ValueError("%s: pulse %d has more than 3 gradient axes" % (who, q))
            b1s.append(b1)
            grs.append(gr)
            tss.append(tp)
            t1s.append(float(t1))
            t2s.append(float(t2))
            gams.append(gamma)
        dfs = [_vec(v) for v in _per_pulse(df, P)]
        dps = []
        for v in _per_pulse(dp, P):
            v = np.asarray(v, dtype=np.float64)
            dps.append(v.reshape(-1, 1) if v.ndim < 2 else v)
        if any(len(v) == 0 for v in dfs) or any(v.shape[0] == 0 or v.shape[1] > 3 for v in dps):
            raise ValueError("%s: an empty grid, or positions with more than 3 axes" % who)
        self.P, self.S, self.sc = P, len(sc), sc
        self.nt = [len(b) for b in b1s]
        self.nf = [len(dfs[0 if len(dfs) == 1 else q]) for q in range(P)]
        self.npos = [dps[0 if len(dps) == 1 else q].shape[0] for q in range(P)]
        gax, pax = max(g.shape[1] for g in grs), max(v.shape[1] for v in dps)
        g3 = [_vec(np.concatenate([g[:, i] if i < g.shape[1] else np.zeros(len(g)) for g in grs])) if i < gax else None
              for i in range(3)]
        p3 = [_vec(np.concatenate([v[:, i] if i < v.shape[1] else np.zeros(v.shape[0]) for v in dps])) if i < pax else None
              for i in range(3)]
        b1 = np.concatenate(b1s)
        nul = C.cast(None, _dp)
        self.keep = [_offsets(self.nt), _vec(b1.real), _vec(b1.imag), g3, _offsets([len(t) for t in tss]), _vec(np.concatenate(tss)),
                     _vec(t1s), _vec(t2s), _vec(gams), _offsets([len(v) for v in dfs]), _vec(np.concatenate(dfs)),
                     _offsets([v.shape[0] for v in dps]), p3]
        k = self.keep
        self.head = [P, _lptr(k[0]), _ptr(k[1]), _ptr(k[2]), *[_ptr(g) if g is not None else nul for g in g3], _lptr(k[4]), _ptr(k[5]),
                     _ptr(k[6]), _ptr(k[7]), _ptr(k[8]), len(dfs), _lptr(k[9]), _ptr(k[10]), len(dps), _lptr(k[11]),
                     *[_ptr(p) if p is not None else nul for p in p3], self.S, _ptr(sc)]

    def m0_planes(self, m0, ooff, ntout):
        """Three planes of ooff[-1] zeros with the initial magnetisation (None: [0 0 1]) at the first entry of every (scale,
        frequency, position) block of ntout[q] entries."""
        out = [np.zeros(int(ooff[-1])) for _ in range(3)]
        each = isinstance(m0, list) and len(m0) == self.P and all(isinstance(t, tuple) and len(t) == 3 for t in m0)
        for c, dflt in enumerate((0.0, 0.0, 1.0)):
            for q in range(self.P):
                v, nf, npos = dflt, self.nf[q], self.npos[q]
                if m0 is not None:
                    v = np.asarray((m0[q] if each else m0)[c], dtype=np.float64)
                    v = v.reshape(nf, npos) if v.size == nf * npos else np.broadcast_to(v, (nf, npos))
                    v = v.ravel()
                out[c][ooff[q]:ooff[q + 1]].reshape(self.S, nf * npos, ntout[q])[:, :, 0] = v
        return out


def bloch_batch(pulses, df, dp, *, scales=(1.0,), mode=0, m0=None, ctx=None):
    """Many `bloch` simulations in one launch (mbfir_bloch_batch): every pulse at every transmit-gain scale.  Each pulse is
    (b1, gr, tp, t1, t2, nucleus) with bloch's meaning of every field (tp a scalar interval, ntime intervals or ntime increasing
    end times; nucleus 'C-13', 'H-1' or gamma in rad/s/G).  df (Hz) and dp (cm, (npos,) or (npos, 1..3)): one grid shared by
    every pulse, or a Python list of one array per pulse.  Scale s multiplies b1.  m0: None (equilibrium) or (mx, my, mz), each
    a scalar or (nf, npos) per pulse, the initial magnetisation at every scale, or a Python list of one such tuple per pulse.  Returns a list of (mx, my, mz) per pulse, each of
    shape (S, nf, npos) or, with mode & 2, (S, nf, npos, ntime).  A pulse's bits depend neither on the other pulses nor on the
    other scales."""
    pulses, sc = list(pulses), _vec(scales)
    if pulses and len(sc) and mode not in (0, 1, 2, 3):
        raise ValueError("bloch_batch: mode must be 0, 1, 2 or 3")
    A = _BlochArgs("bloch_batch", pulses, df, dp, sc)
    P, S, mode, nt, nf, npos = A.P, A.S, int(mode), A.nt, A.nf, A.npos
    ntout = [n if mode & 2 else 1 for n in nt]
    ooff = _offsets([S * f * k * o for f, k, o in zip(nf, npos, ntout)])
    out = A.m0_planes(m0, ooff, ntout)
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_batch(ctx._h, *A.head, mode, *[_ptr(o) for o in out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = []
    for q in range(P):
        shape = (S, nf[q], npos[q], nt[q]) if mode & 2 else (S, nf[q], npos[q])
        res.append(tuple(o[ooff[q]:ooff[q + 1]].reshape(shape) for o in out))
    return res


def _bloch_cotangents(who, cot, A):
    """cot: per pulse (cmx, cmy, cmz), each of shape (S, nf, npos) -> the three concatenated planes of the C call"""
    cot = list(cot)
    if len(cot) != A.P:
        raise ValueError("%s: %d cotangent triples for %d pulses" % (who, len(cot), A.P))
    planes = [[], [], []]
    for q, tri in enumerate(cot):
        if not isinstance(tri, (tuple, list)) or len(tri) != 3:
            raise ValueError("%s: the cotangent of pulse %d must be a triple (cmx, cmy, cmz)" % (who, q))
        tri = [np.asarray(v, dtype=np.float64) for v in tri]
        shape = (A.S, A.nf[q], A.npos[q])
        if any(v.shape != shape for v in tri):
            raise ValueError("%s: the cotangents of pulse %d have shapes %s, %s and %s, the forward call returns %s"
                             % ((who, q) + tuple(v.shape for v in tri) + (shape,)))
        for c in range(3):
            planes[c].append(tri[c].ravel())
    return [_vec(np.concatenate(p)) for p in planes]


def bloch_vjp_batch(pulses, df, dp, cot, *, scales=(1.0,), m0=None, grad_m0=False, ctx=None):
    """The adjoint of bloch_batch's end point (mode 0) with respect to b1 and the initial magnetisation, relaxation included
    (mbfir_bloch_vjp_batch): pulses, df, dp, scales and m0 as for bloch_batch; cot: one (cmx, cmy, cmz) per pulse,
    the cotangents of the (mx, my, mz) that bloch_batch returns, each of shape (S, nf, npos).  Returns a list of complex (ntime,)
    gradients dL/dRe b1 + i dL/dIm b1, summed over the points and the scales; with grad_m0, a list of (grad_b1, (gmx, gmy, gmz)),
    the second being dL/dm0 of every (scale, frequency, position), each of shape (S, nf, npos) (one m0 serves every scale: its
    gradient is their sum over the scales).  Deterministic: a pulse's gradient bits depend only on the pulse, its grids, its
    cotangents and the scales.  gr, tp, t1, t2, df and dp are not differentiated."""
    A = _BlochArgs("bloch_vjp_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    cm = _bloch_cotangents("bloch_vjp_batch", cot, A)
    ooff, toff = _offsets([S * f * k for f, k in zip(nf, npos)]), _offsets(A.nt)
    nul = C.cast(None, _dp)
    m0p = [nul] * 3 if m0 is None else A.m0_planes(m0, ooff, [1] * P)
    grad = [np.zeros(int(toff[-1])) for _ in range(2)]
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_vjp_batch(ctx._h, *A.head, *[_plane(v) if m0 is not None else v for v in m0p],
                                              *[_ptr(v) for v in cm], _ptr(grad[0]), _ptr(grad[1]),
                                              *[_ptr(v) if grad_m0 else v for v in gm])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all = grad[0] + 1j * grad[1]
    res = [g_all[toff[q]:toff[q + 1]] for q in range(P)]
    if not grad_m0:
        return res
    return [(res[q], tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm)) for q in range(P)]


def bloch_vjp_gr_batch(pulses, df, dp, cot, *, scales=(1.0,), m0=None, grad_m0=False, grad_df=False, ctx=None):
    """The adjoint of bloch_batch's end point (mode 0) with respect to b1, the gradient waveform gr and, on request, the initial
    magnetisation and the off-resonance df, relaxation included (mbfir_bloch_vjp_gr_batch): arguments as
    bloch_vjp_batch.  Returns one (grad_b1, grad_gr) per pulse: grad_b1 as bloch_vjp_batch returns it (equal to rounding, not
    promised to the bit), and grad_gr real of shape (ntime, 3), column a = dL/dg_a in the units of gr, summed over the points and
    over the scales without a factor (a scale multiplies b1, not gr); a column whose axis the pulse does not play is the derivative
    at a zero gradient, and is zero only where the positions lack that axis too.  With grad_m0 and / or grad_df further members
    follow in that order: (gmx, gmy, gmz) as bloch_vjp_batch returns it, and grad_df of shape (S, nf, npos), dL/ddf per scale,
    frequency and position: the caller sums over whatever shares an off-resonance.  Deterministic: the bits of every result depend
    only on the pulse, its grids, its cotangents and the scales.  tp, t1, t2, dp and the scales are not differentiated."""
    A = _BlochArgs("bloch_vjp_gr_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    cm = _bloch_cotangents("bloch_vjp_gr_batch", cot, A)
    ooff, toff = _offsets([S * f * k for f, k in zip(nf, npos)]), _offsets(A.nt)
    nul = C.cast(None, _dp)
    m0p = [nul] * 3 if m0 is None else A.m0_planes(m0, ooff, [1] * P)
    grad = [np.zeros(int(toff[-1])) for _ in range(5)]                  # Re, Im of b1; gx, gy, gz
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    gd = np.zeros(int(ooff[-1])) if grad_df else nul
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_vjp_gr_batch(ctx._h, *A.head, *[_plane(v) if m0 is not None else v for v in m0p],
                                                 *[_ptr(v) for v in cm], _ptr(grad[0]), _ptr(grad[1]),
                                                 *[_ptr(v) if grad_m0 else v for v in gm], *[_ptr(v) for v in grad[2:]],
                                                 _ptr(gd) if grad_df else gd)
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all, gg = grad[0] + 1j * grad[1], np.stack(grad[2:], 1)
    res = []
    for q in range(P):
        out = (g_all[toff[q]:toff[q + 1]], gg[toff[q]:toff[q + 1]])
        if grad_m0:
            out += (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm),)
        if grad_df:
            out += (gd[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]),)
        res.append(out)
    return res


def bloch_jvp_batch(pulses, df, dp, tangents, *, scales=(1.0,), m0=None, tangents_m0=None, ctx=None):
    """The tangent of bloch_batch's end point (mode 0) with respect to b1 and the initial magnetisation, relaxation included
    (mbfir_bloch_jvp_batch): pulses, df, dp, scales and m0 as for bloch_batch; tangents: per pulse a complex
    direction of b1 of shape (n,), or K of them of shape (K, n), the same K for every pulse; tangents_m0: None (m0 does not move) or
    per pulse a triple (dmx, dmy, dmz), each broadcastable to (K, nf, npos): the direction of m0 that goes with each b1 direction,
    the same at every scale, as m0 is.  Returns a list of ((mx, my, mz), (dmx, dmy, dmz)) per pulse: the primal of shape (S, nf,
    npos) with bloch_batch's bits, and d/de m(b1 + e v, m0 + e dm0) at e = 0 for each direction, of shape (K, S, nf, npos), without
    the K axis for a 1-D tangent.  Real-linear in (v, dm0).  One launch, the directions sharing each sample's trigonometry and
    rotation; a tangent's bits depend only on its pulse, scale, point and direction.  gr, tp, t1, t2, df and dp are not
    differentiated."""
    A = _BlochArgs("bloch_jvp_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    K, keep, vplanes = _tangents("bloch_jvp_batch", tangents, [range(n) for n in A.nt])
    ooff = _offsets([S * f * k for f, k in zip(nf, npos)])
    nul = C.cast(None, _dp)
    dm0 = [nul] * 3
    if tangents_m0 is not None:
        tangents_m0 = list(tangents_m0)
        if len(tangents_m0) != P:
            raise ValueError("bloch_jvp_batch: %d m0 tangent triples for %d pulses" % (len(tangents_m0), P))
        planes = [[], [], []]
        for q, tri in enumerate(tangents_m0):
            if not isinstance(tri, (tuple, list)) or len(tri) != 3:
                raise ValueError("bloch_jvp_batch: the m0 tangent of pulse %d must be a triple (dmx, dmy, dmz)" % q)
            for c in range(3):
                v = np.asarray(tri[c], dtype=np.float64)
                try:
                    v = np.broadcast_to(v, (K, nf[q], npos[q]))
                except ValueError:
                    raise ValueError("bloch_jvp_batch: an m0 tangent of pulse %d has shape %s, which does not broadcast to %s"
                                     % (q, v.shape, (K, nf[q], npos[q]))) from None
                planes[c].append(np.broadcast_to(v[:, None], (K, S, nf[q], npos[q])).ravel())
        dm0 = [_vec(np.concatenate(p)) for p in planes]
    m0p = [nul] * 3 if m0 is None else A.m0_planes(m0, ooff, [1] * P)
    out = [np.zeros(int(ooff[-1])) for _ in range(3)]
    tan = [np.zeros(K * int(ooff[-1])) for _ in range(3)]
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_jvp_batch(ctx._h, *A.head, *[_plane(v) for v in m0p], K, *[_ptr(v) for v in vplanes],
                                              *[_plane(v) for v in dm0], *[_ptr(v) for v in out], *[_ptr(v) for v in tan])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = []
    for q in range(P):
        lo, hi, shape = int(ooff[q]), int(ooff[q + 1]), (S, nf[q], npos[q])
        res.append((tuple(o[lo:hi].reshape(shape) for o in out),
                    tuple(t[K * lo:K * hi].reshape(((K,) if keep else ()) + shape) for t in tan)))
    return res


def bloch_ss_vjp_batch(pulses, df, dp, cot, *, scales=(1.0,), steady=False, ctx=None):
    """The adjoint of bloch_batch's steady state (mode 1) with respect to b1 (mbfir_bloch_ss_vjp_batch): pulses
    (each one period: for balanced SSFP the pulse plus the dead time of one repetition), df, dp and scales as for bloch_batch; cot:
    one (cmx, cmy, cmz) per pulse, the cotangents of the (mx, my, mz) that bloch_batch(mode=1) returns, each of shape (S, nf, npos).
    Returns a list of complex (ntime,) gradients dL/dRe b1 + i dL/dIm b1, summed over the points and the scales; with steady, a list
    of (grad_b1, (mx, my, mz)), the second being the steady state itself with bloch_batch(mode=1)'s bits, each of shape (S, nf,
    npos).  One upload, two launches, one download.  The steady state does not depend on m0: there is no m0 and no dL/dm0.
    Deterministic: a pulse's gradient bits depend only on the pulse, its grids, its cotangents and the scales.  The error grows with
    ||(I - A)^-1||, about T1 / TR; where the steady state itself is not finite, the gradient is not either.  gr, tp, t1, t2, df and
    dp are not differentiated."""
    A = _BlochArgs("bloch_ss_vjp_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    cm = _bloch_cotangents("bloch_ss_vjp_batch", cot, A)
    ooff, toff = _offsets([S * f * k for f, k in zip(nf, npos)]), _offsets(A.nt)
    nul = C.cast(None, _dp)
    grad = [np.zeros(int(toff[-1])) for _ in range(2)]
    out = [np.zeros(int(ooff[-1])) for _ in range(3)] if steady else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_ss_vjp_batch(ctx._h, *A.head, *[_ptr(v) for v in cm], _ptr(grad[0]), _ptr(grad[1]),
                                                 *[_ptr(v) if steady else v for v in out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all = grad[0] + 1j * grad[1]
    res = [g_all[toff[q]:toff[q + 1]] for q in range(P)]
    if not steady:
        return res
    return [(res[q], tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in out)) for q in range(P)]


def bloch_ss_vjp_gr_batch(pulses, df, dp, cot, *, scales=(1.0,), grad_df=False, steady=False, ctx=None):
    """The adjoint of bloch_batch's steady state (mode 1) with respect to b1, the gradient waveform gr and, on request, the
    off-resonance df (mbfir_bloch_ss_vjp_gr_batch): arguments as bloch_ss_vjp_batch.  Returns one (grad_b1,
    grad_gr) per pulse: grad_b1 as bloch_ss_vjp_batch returns it (equal to rounding, not promised to the bit), and grad_gr real of
    shape (ntime, 3), column a = dL/dg_a in the units of gr, summed over the points and over the scales without a factor (a scale
    multiplies b1, not gr); a column whose axis the pulse does not play is the derivative at a zero gradient.  With grad_df and / or
    steady further members follow in that order: grad_df of shape (S, nf, npos), dL/ddf per scale, frequency and position (the
    caller sums over whatever shares an off-resonance), and (mx, my, mz), the steady state itself with bloch_batch(mode=1)'s bits.
    One upload, two launches, one download.  There is no m0 and no dL/dm0.  Deterministic: the bits of every result depend only on
    the pulse, its grids, its cotangents and the scales.  The error grows with ||(I - A)^-1||, about T1 / TR, grad_df's with its
    square.  tp, t1, t2, dp and the scales are not differentiated."""
    A = _BlochArgs("bloch_ss_vjp_gr_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    cm = _bloch_cotangents("bloch_ss_vjp_gr_batch", cot, A)
    ooff, toff = _offsets([S * f * k for f, k in zip(nf, npos)]), _offsets(A.nt)
    nul = C.cast(None, _dp)
    grad = [np.zeros(int(toff[-1])) for _ in range(5)]                  # Re, Im of b1; gx, gy, gz
    out = [np.zeros(int(ooff[-1])) for _ in range(3)] if steady else [nul] * 3
    gd = np.zeros(int(ooff[-1])) if grad_df else nul
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_ss_vjp_gr_batch(ctx._h, *A.head, *[_ptr(v) for v in cm], _ptr(grad[0]), _ptr(grad[1]),
                                                    *[_ptr(v) if steady else v for v in out], *[_ptr(v) for v in grad[2:]],
                                                    _ptr(gd) if grad_df else gd)
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all, gg = grad[0] + 1j * grad[1], np.stack(grad[2:], 1)
    res = []
    for q in range(P):
        r = (g_all[toff[q]:toff[q + 1]], gg[toff[q]:toff[q + 1]])
        if grad_df:
            r += (gd[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]),)
        if steady:
            r += (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in out),)
        res.append(r)
    return res


def bloch_ss_jvp_batch(pulses, df, dp, tangents, *, scales=(1.0,), ctx=None):
    """The tangent of bloch_batch's steady state (mode 1) with respect to b1 (mbfir_bloch_ss_jvp_batch): pulses,
    df, dp and scales as for bloch_batch; tangents: per pulse a complex direction of b1 of shape (n,), or K of them of shape (K, n),
    the same K for every pulse.  Returns a list of ((mx, my, mz), (dmx, dmy, dmz)) per pulse: the steady state of shape (S, nf,
    npos) with bloch_batch(mode=1)'s bits, and d/de M(b1 + e v) at e = 0 for each direction, of shape (K, S, nf, npos), without the K
    axis for a 1-D tangent.  Real-linear in v.  One launch; a tangent's bits depend only on its pulse, scale, point and direction.
    gr, tp, t1, t2, df and dp are not differentiated."""
    A = _BlochArgs("bloch_ss_jvp_batch", pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    K, keep, vplanes = _tangents("bloch_ss_jvp_batch", tangents, [range(n) for n in A.nt])
    ooff = _offsets([S * f * k for f, k in zip(nf, npos)])
    out = [np.zeros(int(ooff[-1])) for _ in range(3)]
    tan = [np.zeros(K * int(ooff[-1])) for _ in range(3)]
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_ss_jvp_batch(ctx._h, *A.head, K, *[_ptr(v) for v in vplanes], *[_ptr(v) for v in out],
                                                 *[_ptr(v) for v in tan])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = []
    for q in range(P):
        lo, hi, shape = int(ooff[q]), int(ooff[q + 1]), (S, nf[q], npos[q])
        res.append((tuple(o[lo:hi].reshape(shape) for o in out),
                    tuple(t[K * lo:K * hi].reshape(((K,) if keep else ()) + shape) for t in tan)))
    return res


def _bloch_planes(who, what, triples, A, weights=False, magnitude=False):
    """triples: per pulse (x, y, z), each of shape (S, nf, npos), or (nf, npos) for every scale, or a scalar -> the three
    concatenated planes of the C call in the layout of bloch_batch's mode-0 outputs; magnitude: per pulse a pair (xy, z) -> the two
    planes of the magnitude calls"""
    triples = list(triples)
    n, form = (2, "pair (xy, z)") if magnitude else (3, "triple (x, y, z)")
    if len(triples) != A.P:
        raise ValueError("%s: %d %s %ss for %d pulses" % (who, len(triples), what, form.split()[0], A.P))
    planes = [[] for _ in range(n)]
    for q, tri in enumerate(triples):
        if not isinstance(tri, (tuple, list)) or len(tri) != n:
            raise ValueError("%s: the %ss of pulse %d must be a %s" % (who, what, q, form))
        shape = (A.S, A.nf[q], A.npos[q])
        for c in range(n):
            v = np.asarray(tri[c], dtype=np.float64)
            if v.shape != shape and v.shape != shape[1:] and v.shape != ():
                raise ValueError("%s: a %s of pulse %d has shape %s, not %s, %s or a scalar" % (who, what, q, v.shape, shape, shape[1:]))
            if weights and (not np.all(np.isfinite(v)) or np.any(v < 0)):
                raise ValueError("%s: a weight of pulse %d is negative or not finite" % (who, q))
            planes[c].append(np.broadcast_to(v, shape).ravel())
    return [_vec(np.concatenate(p)) for p in planes]


def _bloch_m0(A, m0):
    """The m0 of the least-squares calls: three NULLs, or the planes of the mode-0 layout (arrays: the caller keeps them alive)"""
    if m0 is None:
        return [C.cast(None, _dp)] * 3
    return A.m0_planes(m0, _offsets([A.S * f * k for f, k in zip(A.nf, A.npos)]), [1] * A.P)


# ---- pulse trains: the echo-by-echo transient of N repetitions of a period (mbfir_bloch_train_batch) ----------
def _train_ints(who, what, v, P, default=None):
    """ntr / echo: None (the default per pulse), an int for every pulse, or a list of one int per pulse -> a list of P ints"""
    if v is None:
        return list(default)
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != P:
            raise ValueError("%s: %d values of %s for %d pulses" % (who, len(v), what, P))
        v = list(v)
    else:
        v = [v] * P
    if any(int(e) != e for e in v):
        raise ValueError("%s: %s must be an integer" % (who, what))
    return [int(e) for e in v]


def _train_echo(who, echo, A):
    echo = _train_ints(who, "echo", echo, A.P, A.nt)
    for q, (e, n) in enumerate(zip(echo, A.nt)):
        if e < 0 or e > n:
            raise ValueError("%s: echo of pulse %d must lie in [0, ntime]" % (who, q))
    return np.ascontiguousarray(echo, dtype=np.int32)


def _train_tables(who, what, v, ntr, increment):
    """phases / gains: a scalar (increment: phi_k = k v; else the value of every repetition), an array of ntr values for every
    pulse, or a Python list of one array per pulse -> a list of P float64 arrays of ntr[q] values"""
    P = len(ntr)
    each = _per_pulse(v, P)
    out = []
    for q, n in enumerate(ntr):
        e = np.asarray(each[0 if len(each) == 1 else q], dtype=np.float64)
        if e.ndim == 0:
            e = np.arange(n) * float(e) if increment else np.full(n, float(e))
        e = e.ravel()
        if len(e) != n:
            raise ValueError("%s: %s of pulse %d has %d entries for its %d repetitions" % (who, what, q, len(e), n))
        out.append(e)
    return out


class _TrainArgs:
    """The arguments that bloch_train_batch and its adjoint share, checked and laid out for the C calls: A (_BlochArgs), ntr (a list),
    tail (the C arguments from ntr through demod), ooff (the final planes' offsets) and eoff (the echo planes')"""

    def __init__(self, who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod):
        A = _BlochArgs(who, pulses, df, dp, scales)
        P, S, nf, npos = A.P, A.S, A.nf, A.npos
        ntr = _train_ints(who, "ntr", ntr, P)
        for q, n in enumerate(ntr):
            if n < 1:
                raise ValueError("%s: ntr of pulse %d must be at least 1" % (who, q))
        ech = _train_echo(who, echo, A)
        ph, gn = _train_tables(who, "phases", phases, ntr, True), _train_tables(who, "gains", gains, ntr, False)
        if not all(np.all(np.isfinite(g)) for g in gn):
            raise ValueError("%s: a gain is not finite" % who)
        if not all(np.all(np.isfinite(p)) for p in ph):
            raise ValueError("%s: a cosine or sine of the phase table is not finite" % who)
        mq = _vec(meq)
        if mq.size not in (1, P):
            raise ValueError("%s: %d values of meq for %d pulses" % (who, mq.size, P))
        mq = np.ascontiguousarray(np.broadcast_to(mq, (P,)))
        for q in range(P):
            if not np.isfinite(mq[q]):
                raise ValueError("%s: meq of pulse %d is not finite" % (who, q))
        uniq = [np.unique(g, return_inverse=True) for g in gn]             # the distinct gains and every repetition's index among them
        phi = np.concatenate(ph)
        cs, sn = _vec(np.cos(phi)), _vec(np.sin(phi))
        gidx = np.ascontiguousarray(np.concatenate([u[1].ravel() for u in uniq]), dtype=np.int32)
        gains_d = _vec(np.concatenate([u[0] for u in uniq]))
        ntr_a, roff, goff = np.ascontiguousarray(ntr, dtype=np.int32), _offsets(ntr), _offsets([len(u[0]) for u in uniq])
        ooff = _offsets([S * f * k for f, k in zip(nf, npos)])
        eoff = _offsets([S * n * f * k for n, f, k in zip(ntr, nf, npos)])
        self.A, self.ntr, self.ooff, self.eoff = A, ntr, ooff, eoff
        self._keep = (ntr_a, roff, cs, sn, gidx, goff, gains_d, ech, mq)                     # the arrays behind the pointers
        self.tail = [ntr_a.ctypes.data_as(_ip), _lptr(roff), _ptr(cs), _ptr(sn), gidx.ctypes.data_as(_ip), _lptr(goff), _ptr(gains_d),
                     ech.ctypes.data_as(_ip), _ptr(mq), int(bool(demod))]


def bloch_train_batch(pulses, df, dp, ntr, *, phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False,
                      final=False, ctx=None):
    """The echo-by-echo transient of pulse trains (mbfir_bloch_train_batch).  Each pulse is one period, exactly
    as bloch_batch takes it (dead time as zero-b1 samples with their own tp); a train plays it ntr times (an int, or a list of one
    int per pulse), repetition k at gains[k] exp(i phases[k]) b1 with the gradients and the timing of the period.  phases: a scalar
    increment D, phi_k = k D (the default pi is alternating bSSFP), an array of ntr phases in radians, or a Python list of one such
    array per pulse.  gains: a scalar, an array of ntr values (a catalysation ramp, a variable-flip-angle schedule), or a Python
    list of one array per pulse.  echo: the sample index in [0, ntime] after which the echo is read, an int or a list of one per
    pulse; None = ntime, the state at the end of each repetition.  df, dp, scales and m0 as for bloch_batch.  meq (a scalar or one
    per pulse) scales every recovery term (1 - E1): 1 is bloch's convention, 0 the hyperpolarised limit, in which the train is
    linear in m0.  demod: return the echoes in the frame of each repetition's RF phase.  Returns, per pulse, (mx, my, mz) of shape
    (S, ntr, nf, npos); with final, ((mx, my, mz), (fx, fy, fz)), the second being the magnetisation after the last repetition, of
    shape (S, nf, npos), which a following train takes as m0.  The period is swept once per (scale, distinct gain); a repetition
    then costs about sixty flops per point.  Deterministic: a result's bits depend only on its pulse, scale, point and train, and
    the first n echoes of a train are those of the train cut after n repetitions."""
    Tn = _TrainArgs("bloch_train_batch", pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff, eoff = Tn.A, Tn.ntr, Tn.ooff, Tn.eoff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    m0p = _bloch_m0(A, m0)
    out = [np.zeros(int(eoff[-1])) for _ in range(3)]
    fin = [np.zeros(int(ooff[-1])) for _ in range(3)] if final else [C.cast(None, _dp)] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], *[_ptr(v) for v in out],
                                                *[_plane(v) for v in fin])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = []
    for q in range(P):
        e = tuple(o[eoff[q]:eoff[q + 1]].reshape(S, ntr[q], nf[q], npos[q]) for o in out)
        res.append((e, tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in fin)) if final else e)
    return res


def bloch_prop_batch(pulses, df, dp, *, echo=None, scales=(1.0,), ctx=None):
    """The propagators of one period (mbfir_bloch_prop_batch, the first launch of bloch_train_batch on its own): pulses, df, dp,
    scales and echo as for bloch_train_batch.  Returns, per pulse, (A, B, Ae, Be): one period is m -> A m + B at RF phase 0 (B at
    meq = 1), its first `echo` samples m -> Ae m + Be; A and Ae of shape (S, nf, npos, 3, 3), B and Be of shape (S, nf, npos, 3).
    Periods compose on the host: (A2, B2) after (A1, B1) is (A2 A1, A2 B1 + B2)."""
    who = "bloch_prop_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    ech = _train_echo(who, echo, A)
    ooff = _offsets([S * f * k for f, k in zip(nf, npos)])
    O = int(ooff[-1])
    a, b, ae, be = np.zeros(9 * O), np.zeros(3 * O), np.zeros(9 * O), np.zeros(3 * O)
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_prop_batch(ctx._h, *A.head, ech.ctypes.data_as(_ip), _ptr(a), _ptr(b), _ptr(ae), _ptr(be))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = []
    for q in range(P):
        lo, hi, shape = int(ooff[q]), int(ooff[q + 1]), (S, nf[q], npos[q])
        mat = lambda v: v[9 * lo:9 * hi].reshape(shape + (3, 3)).swapaxes(-1, -2)          # column-major: entry (i, j) at i + 3 j
        res.append((mat(a), b[3 * lo:3 * hi].reshape(shape + (3,)), mat(ae), be[3 * lo:3 * hi].reshape(shape + (3,))))
    return res


def _train_cotangents(who, what, cot, A, lead):
    """cot: None, or per pulse (cx, cy, cz), each of shape (S,) + lead[q] + (nf, npos) -> None or the three concatenated planes"""
    if cot is None:
        return None
    cot = list(cot)
    if len(cot) != A.P:
        raise ValueError("%s: %d %s cotangent triples for %d pulses" % (who, len(cot), what, A.P))
    planes = [[], [], []]
    for q, tri in enumerate(cot):
        if not isinstance(tri, (tuple, list)) or len(tri) != 3:
            raise ValueError("%s: the %s cotangent of pulse %d must be a triple (cx, cy, cz)" % (who, what, q))
        tri = [np.asarray(v, dtype=np.float64) for v in tri]
        shape = (A.S,) + lead[q] + (A.nf[q], A.npos[q])
        if any(v.shape != shape for v in tri):
            raise ValueError("%s: the %s cotangents of pulse %d have shapes %s, %s and %s, the forward call returns %s"
                             % ((who, what, q) + tuple(v.shape for v in tri) + (shape,)))
        for c in range(3):
            planes[c].append(tri[c].ravel())
    return [_vec(np.concatenate(p)) for p in planes]


def bloch_train_vjp_batch(pulses, df, dp, ntr, cot, *, cot_final=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None,
                          meq=1.0, demod=False, grad_m0=False, ctx=None):
    """The adjoint of bloch_train_batch with respect to b1 and the initial magnetisation (mbfir_bloch_train_vjp_batch, DESIGN
    section 8z): pulses, df, dp, ntr, phases, gains, echo, scales, m0, meq and demod as for bloch_train_batch.  cot: None, or one
    (cx, cy, cz) per pulse, the cotangents of the echoes that bloch_train_batch returns, each of shape (S, ntr, nf, npos);
    cot_final: None, or one (cx, cy, cz) per pulse, the cotangents of the final state, each of shape (S, nf, npos); not both None.
    Returns a list of complex (ntime,) gradients dL/dRe b1 + i dL/dIm b1 of the period's samples, summed over the points, the
    scales and the repetitions (repetition k plays gains[k] exp(i phases[k]) b1: that factor's chain rule is included); with
    grad_m0, a list of (grad_b1, (gmx, gmy, gmz)), the second being dL/dm0 of every (scale, frequency, position), each of shape
    (S, nf, npos) (one m0 serves every scale: its gradient is their sum over the scales).  One upload, four launches, one
    download; the cost is a small multiple of the forward train's.  Deterministic: a pulse's gradient bits depend only on the
    pulse, its grids, its train, its cotangents and the scales, and dL/dm0 has the same bits for any m0 and any meq.  gr, tp,
    t1, t2, df, dp and meq are not differentiated (the gains and the phases: bloch_train_vjp_sched_batch)."""
    who = "bloch_train_vjp_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff, eoff = Tn.A, Tn.ntr, Tn.ooff, Tn.eoff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if cot is None and cot_final is None:
        raise ValueError("%s: neither echo cotangents nor final cotangents are given" % who)
    ce = _train_cotangents(who, "echo", cot, A, [(n,) for n in ntr])
    cf = _train_cotangents(who, "final", cot_final, A, [()] * P)
    toff = _offsets(A.nt)
    nul = C.cast(None, _dp)
    m0p = _bloch_m0(A, m0)
    grad = [np.zeros(int(toff[-1])) for _ in range(2)]
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_vjp_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p],
                                                    *([nul] * 3 if ce is None else [_ptr(v) for v in ce]),
                                                    *([nul] * 3 if cf is None else [_ptr(v) for v in cf]), _ptr(grad[0]),
                                                    _ptr(grad[1]), *[_plane(v) for v in gm])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all = grad[0] + 1j * grad[1]
    res = [g_all[toff[q]:toff[q + 1]] for q in range(P)]
    if not grad_m0:
        return res
    return [(res[q], tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm)) for q in range(P)]


def bloch_train_vjp_gr_batch(pulses, df, dp, ntr, cot, *, cot_final=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None,
                             meq=1.0, demod=False, grad_m0=False, grad_df=False, ctx=None):
    """The adjoint of bloch_train_batch with respect to b1, the gradient waveform gr of the period and, on request, the initial
    magnetisation and the off-resonance df (mbfir_bloch_train_vjp_gr_batch): arguments as
    bloch_train_vjp_batch.  Returns one (grad_b1, grad_gr) per pulse: grad_b1 as bloch_train_vjp_batch returns it (equal to
    rounding, not promised to the bit), and grad_gr real of shape (ntime, 3), column a = dL/dg_a of the period's samples in the
    units of gr, summed over the points, the repetitions, the scales and the gains without a factor (scale and gain multiply b1,
    not gr); a column whose axis the pulse does not play is the derivative at a zero gradient, and is exactly zero where the
    positions lack that axis too.  With grad_m0 and / or grad_df further members follow in that order: (gmx, gmy, gmz) with
    bloch_train_vjp_batch's bits, and grad_df of shape (S, nf, npos), dL/ddf per scale, frequency and position, summed over the
    repetitions: the caller sums over whatever shares an off-resonance.  One upload, four launches (five with grad_df), one
    download.  Deterministic: the bits of every result depend only on the pulse, its grids, its train, its cotangents and the
    scales.  tp, t1, t2, dp, meq and the scales are not differentiated (the gains and the phases: bloch_train_vjp_sched_batch)."""
    who = "bloch_train_vjp_gr_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff = Tn.A, Tn.ntr, Tn.ooff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if cot is None and cot_final is None:
        raise ValueError("%s: neither echo cotangents nor final cotangents are given" % who)
    ce = _train_cotangents(who, "echo", cot, A, [(n,) for n in ntr])
    cf = _train_cotangents(who, "final", cot_final, A, [()] * P)
    toff = _offsets(A.nt)
    nul = C.cast(None, _dp)
    m0p = _bloch_m0(A, m0)
    grad = [np.zeros(int(toff[-1])) for _ in range(5)]                  # Re, Im of b1; gx, gy, gz
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    gd = np.zeros(int(ooff[-1])) if grad_df else nul
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_vjp_gr_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p],
                                                       *([nul] * 3 if ce is None else [_ptr(v) for v in ce]),
                                                       *([nul] * 3 if cf is None else [_ptr(v) for v in cf]), _ptr(grad[0]),
                                                       _ptr(grad[1]), *[_plane(v) for v in gm], *[_ptr(v) for v in grad[2:]],
                                                       _ptr(gd) if grad_df else gd)
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    g_all, gg = grad[0] + 1j * grad[1], np.stack(grad[2:], 1)
    res = []
    for q in range(P):
        out = (g_all[toff[q]:toff[q + 1]], gg[toff[q]:toff[q + 1]])
        if grad_m0:
            out += (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm),)
        if grad_df:
            out += (gd[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]),)
        res.append(out)
    return res


def bloch_train_vjp_sched_batch(pulses, df, dp, ntr, cot, *, cot_final=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,),
                                m0=None, meq=1.0, demod=False, grad_gains=True, grad_phases=True, grad_m0=False, ctx=None):
    """The adjoint of bloch_train_batch with respect to its schedule, the gain and the RF phase of every repetition
    (mbfir_bloch_train_vjp_sched_batch): every argument through demod as for bloch_train_vjp_batch, the loss
    being L = sum_k <cot_k, echo_k> + <cot_final, m_N>.  Returns, per pulse, (grad_gains, grad_phases): dL/dgains[k] and
    dL/dphases[k] (per radian) of every repetition, float64 of shape (ntr,), summed over the scales and the points; None in the
    place of one that was not asked for (not both).  With grad_m0 a third item (gmx, gmy, gmz), dL/dm0 of shape (S, nf, npos) with
    bloch_train_vjp_batch's bits.  The gradients are per repetition whatever form the schedule was given in: repetitions that
    share a gain value still have one entry each, and a scalar `gains` (every repetition at g) or a scalar `phases` increment D
    (phi_k = k D) yields ntr entries g[k], through which the scalar's own derivative follows by the chain rule, dL/dg = sum_k g[k]
    and dL/dD = sum_k k g[k].  A gain of exactly 0 has a finite derivative.  One upload, three launches and a fold (the period is
    swept once more per (scale, distinct gain) for the gains, not at all for the phases), one download: cheaper than
    bloch_train_vjp_batch, which sweeps the period backwards as well.  Deterministic: a pulse's bits depend only on the pulse, its
    grids, its train, its cotangents and the scales, not on what else was asked for.  b1, gr, tp, t1, t2, df, dp and meq are not
    differentiated here."""
    who = "bloch_train_vjp_sched_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff = Tn.A, Tn.ntr, Tn.ooff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if cot is None and cot_final is None:
        raise ValueError("%s: neither echo cotangents nor final cotangents are given" % who)
    if not grad_gains and not grad_phases:
        raise ValueError("%s: neither the gradient in the gains nor the gradient in the phases is wanted" % who)
    ce = _train_cotangents(who, "echo", cot, A, [(n,) for n in ntr])
    cf = _train_cotangents(who, "final", cot_final, A, [()] * P)
    roff = _offsets(ntr)
    nul = C.cast(None, _dp)
    m0p = _bloch_m0(A, m0)
    gg = np.zeros(int(roff[-1])) if grad_gains else None
    gp = np.zeros(int(roff[-1])) if grad_phases else None
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_vjp_sched_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p],
                                                          *([nul] * 3 if ce is None else [_ptr(v) for v in ce]),
                                                          *([nul] * 3 if cf is None else [_ptr(v) for v in cf]),
                                                          nul if gg is None else _ptr(gg), nul if gp is None else _ptr(gp),
                                                          *[_plane(v) for v in gm])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    cut = lambda v, q: None if v is None else v[roff[q]:roff[q + 1]].copy()
    res = [(cut(gg, q), cut(gp, q)) for q in range(P)]
    if not grad_m0:
        return res
    return [res[q] + (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm),) for q in range(P)]


def _train_tangents_m0(who, tangents_m0, A, K):
    """tangents_m0: per pulse a triple (dmx, dmy, dmz), each broadcastable to (K, nf, npos), the same at every scale -> the three
    concatenated planes of the C call, (direction, scale, frequency, position) per pulse"""
    tangents_m0 = list(tangents_m0)
    if len(tangents_m0) != A.P:
        raise ValueError("%s: %d m0 tangent triples for %d pulses" % (who, len(tangents_m0), A.P))
    planes = [[], [], []]
    for q, tri in enumerate(tangents_m0):
        if not isinstance(tri, (tuple, list)) or len(tri) != 3:
            raise ValueError("%s: the m0 tangent of pulse %d must be a triple (dmx, dmy, dmz)" % (who, q))
        shape = (K, A.nf[q], A.npos[q])
        for c in range(3):
            v = np.asarray(tri[c], dtype=np.float64)
            try:
                v = np.broadcast_to(v, shape)
            except ValueError:
                raise ValueError("%s: an m0 tangent of pulse %d has shape %s, which does not broadcast to %s"
                                 % (who, q, v.shape, shape)) from None
            planes[c].append(np.broadcast_to(v[:, None], (K, A.S) + shape[1:]).ravel())
    return [_vec(np.concatenate(p)) for p in planes]


def bloch_train_jvp_batch(pulses, df, dp, ntr, tangents, *, tangents_m0=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,),
                          m0=None, meq=1.0, demod=False, echoes=True, final=False, primal=False, ctx=None):
    """The tangent of bloch_train_batch with respect to b1 and the initial magnetisation (mbfir_bloch_train_jvp_batch, DESIGN
    section 8aa): pulses, df, dp, ntr, phases, gains, echo, scales, m0, meq and demod as for bloch_train_batch.  tangents: per pulse a
    complex direction of the period's b1 of shape (n,), or K of them of shape (K, n), the same K for every pulse (repetition k plays
    gains[k] exp(i phases[k]) (b1 + e v): that factor's chain rule is included); tangents_m0: None (m0 does not move) or per pulse
    a triple (dmx, dmy, dmz), each broadcastable to (K, nf, npos): the direction of m0 that goes with each b1 direction, the same at
    every scale, as m0 is.  Returns, per pulse, the tangent echoes (dex, dey, dez), d/de of the echoes at e = 0, each of shape (K, S,
    ntr, nf, npos), without the K axis for a 1-D tangent; with final, ((dex, dey, dez), (dfx, dfy, dfz)), the second being the
    tangent of the state after the last repetition, each of shape (K, S, nf, npos); with echoes=False (which requires final) the
    final tangents alone.  With primal, per pulse (primal, tangent), the primal being what bloch_train_batch returns for the same
    final (with echoes=False: its final state alone), with its bits.  Real-linear in (v, dm0).  One upload, three launches, one
    download; a tangent's bits depend only on its pulse, scale, point, train and direction.  The gains, the phases, gr, tp, t1, t2,
    df, dp and meq are not differentiated."""
    who = "bloch_train_jvp_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff, eoff = Tn.A, Tn.ntr, Tn.ooff, Tn.eoff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if not echoes and not final:
        raise ValueError("%s: echoes=False requires final=True: neither the tangent echoes nor the final tangents are wanted" % who)
    K, keep, vplanes = _tangents(who, tangents, [range(n) for n in A.nt])
    nul = C.cast(None, _dp)
    dm0 = [nul] * 3 if tangents_m0 is None else _train_tangents_m0(who, tangents_m0, A, K)
    m0p = _bloch_m0(A, m0)
    E, O = int(eoff[-1]), int(ooff[-1])
    pe = [np.zeros(E) for _ in range(3)] if primal and echoes else [nul] * 3
    pf = [np.zeros(O) for _ in range(3)] if primal and final else [nul] * 3
    te = [np.zeros(K * E) for _ in range(3)] if echoes else [nul] * 3
    tf = [np.zeros(K * O) for _ in range(3)] if final else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_jvp_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], K, *[_ptr(v) for v in vplanes],
                                                    *[_plane(v) for v in dm0], *[_plane(v) for v in pe], *[_plane(v) for v in pf],
                                                    *[_plane(v) for v in te], *[_plane(v) for v in tf])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)

    def pick(ev, fv, k, lead, q):
        """The echo and final planes of pulse q, k directions in front with the axes `lead` -> what the flags ask for"""
        e = tuple(v[k * eoff[q]:k * eoff[q + 1]].reshape(lead + (S, ntr[q], nf[q], npos[q])) for v in ev) if echoes else None
        f = tuple(v[k * ooff[q]:k * ooff[q + 1]].reshape(lead + (S, nf[q], npos[q])) for v in fv) if final else None
        return (e, f) if echoes and final else e if echoes else f
    res = []
    for q in range(P):
        tan = pick(te, tf, K, (K,) if keep else (), q)
        res.append((pick(pe, pf, 1, (), q), tan) if primal else tan)
    return res


def _train_tangents_sched(who, what, v, ntr):
    """tangents_gains / tangents_phases: per pulse a float64 direction of shape (ntr,) or (K, ntr) -> (K, keep, a list of (K, ntr)
    arrays); keep: whether the result has the K axis"""
    v = list(v)
    if len(v) != len(ntr):
        raise ValueError("%s: %d %s tangents for %d pulses" % (who, len(v), what, len(ntr)))
    out, K, keep = [], None, False
    for q, (d, n) in enumerate(zip(v, ntr)):
        d = np.asarray(d)
        if np.iscomplexobj(d):
            raise ValueError("%s: the %s tangent of pulse %d is complex; a schedule's direction is real" % (who, what, q))
        d = np.asarray(d, dtype=np.float64)
        if d.ndim not in (1, 2) or d.shape[-1] != n:
            raise ValueError("%s: the %s tangent of pulse %d has shape %s, not (%d,) or (K, %d)" % (who, what, q, d.shape, n, n))
        if q == 0:
            keep, K = d.ndim == 2, d.shape[0] if d.ndim == 2 else 1
        elif (d.ndim == 2) != keep or (keep and d.shape[0] != K):
            raise ValueError("%s: the %s tangent of pulse %d has shape %s; every pulse takes the same K" % (who, what, q, d.shape))
        if K < 1:
            raise ValueError("%s: no directions" % who)
        out.append(d.reshape(K, n))
    return K, keep, out


def bloch_train_jvp_sched_batch(pulses, df, dp, ntr, *, tangents_gains=None, tangents_phases=None, tangents_m0=None, phases=np.pi,
                                gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, echoes=True, final=False,
                                primal=False, ctx=None):
    """The tangent of bloch_train_batch with respect to its schedule, the gain and the RF phase of every repetition, and the initial
    magnetisation (mbfir_bloch_train_jvp_sched_batch): pulses, df, dp, ntr, phases, gains, echo, scales, m0, meq
    and demod as for bloch_train_batch.  tangents_gains / tangents_phases: None (that part does not move) or per pulse a float64
    direction of shape (ntr,), or K of them of shape (K, ntr), the same K for every pulse and for both; the phases' direction is per
    radian.  A direction is per repetition whatever form the schedule was given in: for a scalar `gains` g pass np.ones(ntr), for a
    scalar `phases` increment D pass np.arange(ntr).  tangents_m0: as bloch_train_jvp_batch's.  Not all three None.  Returns what
    bloch_train_jvp_batch returns, with the same shapes and the same echoes / final / primal rules.  With the 2 ntr unit directions
    the result is the whole Jacobian (bloch_train_jacobian_sched_batch).  A gain of exactly 0 is an ordinary case.  One upload, three
    launches (two without tangents_gains), one download: the period is swept once more per (scale, distinct gain) whatever K is,
    and a direction costs two 3 x 3 products per repetition and point.  Real-linear in the direction; a tangent's bits depend only
    on its pulse, scale, point, train and direction, not on K, on its place among the directions or on which parts are None.  b1,
    gr, tp, t1, t2, df, dp and meq are not differentiated here."""
    who = "bloch_train_jvp_sched_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff, eoff = Tn.A, Tn.ntr, Tn.ooff, Tn.eoff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if not echoes and not final:
        raise ValueError("%s: echoes=False requires final=True: neither the tangent echoes nor the final tangents are wanted" % who)
    if tangents_gains is None and tangents_phases is None and tangents_m0 is None:
        raise ValueError("%s: no direction is given: tangents_gains, tangents_phases and tangents_m0 are all None" % who)
    K, keep, parts = None, False, []
    for what, v in (("gains", tangents_gains), ("phases", tangents_phases)):
        if v is None:
            parts.append(None)
            continue
        k, kp, d = _train_tangents_sched(who, what, v, ntr)
        if K is not None and (k, kp) != (K, keep):
            raise ValueError("%s: %d directions of the phases for %d of the gains" % (who, k, K))
        K, keep = k, kp
        parts.append(_vec(np.concatenate([x.ravel() for x in d])))
    if K is None:                                                                # m0 alone: K from its leading axis
        lead = np.asarray(list(tangents_m0)[0][0]) if len(list(tangents_m0)) else np.zeros(())
        keep = lead.ndim == 3
        K = lead.shape[0] if keep else 1
    nul = C.cast(None, _dp)
    dm0 = [nul] * 3 if tangents_m0 is None else _train_tangents_m0(who, tangents_m0, A, K)
    m0p = _bloch_m0(A, m0)
    E, O = int(eoff[-1]), int(ooff[-1])
    pe = [np.zeros(E) for _ in range(3)] if primal and echoes else [nul] * 3
    pf = [np.zeros(O) for _ in range(3)] if primal and final else [nul] * 3
    te = [np.zeros(K * E) for _ in range(3)] if echoes else [nul] * 3
    tf = [np.zeros(K * O) for _ in range(3)] if final else [nul] * 3
    ctx = ctx or get_context()
    rc = load_library().mbfir_bloch_train_jvp_sched_batch(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], K,
                                                          *[nul if v is None else _ptr(v) for v in parts], *[_plane(v) for v in dm0],
                                                          *[_plane(v) for v in pe], *[_plane(v) for v in pf],
                                                          *[_plane(v) for v in te], *[_plane(v) for v in tf])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)

    def pick(ev, fv, k, lead, q):
        """The echo and final planes of pulse q, k directions in front with the axes `lead` -> what the flags ask for"""
        e = tuple(v[k * eoff[q]:k * eoff[q + 1]].reshape(lead + (S, ntr[q], nf[q], npos[q])) for v in ev) if echoes else None
        f = tuple(v[k * ooff[q]:k * ooff[q + 1]].reshape(lead + (S, nf[q], npos[q])) for v in fv) if final else None
        return (e, f) if echoes and final else e if echoes else f
    res = []
    for q in range(P):
        tan = pick(te, tf, K, (K,) if keep else (), q)
        res.append((pick(pe, pf, 1, (), q), tan) if primal else tan)
    return res


def bloch_train_jacobian_sched_batch(pulses, df, dp, ntr, **kw):
    """The whole Jacobian of bloch_train_batch in its schedule: one bloch_train_jvp_sched_batch call with the 2 ntr unit directions,
    the ntr of the gains first, then the ntr of the phases (per radian).  The pulses of a call share ntr (an int).  Keywords as
    bloch_train_jvp_sched_batch's, without the tangents.  Returns what that call returns, the leading axis of length 2 ntr: row j <
    ntr is d/dgains[j], row ntr + j is d/dphases[j]."""
    who = "bloch_train_jacobian_sched_batch"
    for k in ("tangents_gains", "tangents_phases", "tangents_m0"):
        if k in kw:
            raise ValueError("%s: %s is not an argument: the directions are the unit directions of the schedule" % (who, k))
    P = len(list(pulses))
    n = _train_ints(who, "ntr", ntr, P)
    if P == 0 or any(e != n[0] for e in n):
        raise ValueError("%s: the pulses of a call must share ntr" % who)
    if n[0] < 1:
        raise ValueError("%s: ntr of pulse 0 must be at least 1" % who)
    eye, zero = np.eye(n[0]), np.zeros((n[0], n[0]))
    return bloch_train_jvp_sched_batch(pulses, df, dp, ntr, tangents_gains=[np.concatenate([eye, zero])] * P,
                                       tangents_phases=[np.concatenate([zero, eye])] * P, **kw)


def bloch_lsq_batch(pulses, df, dp, targets, weights, *, scales=(1.0,), m0=None, magnitude=False, ctx=None):
    """Loss and gradient of a weighted least-squares fit of bloch_batch's end point (mode 0), relaxation included, in one device
    call (mbfir_bloch_lsq_batch): pulses, df, dp, scales and m0 as for bloch_batch.  targets and weights: per
    pulse a triple (x, y, z) for (mx, my, mz), each entry of the shape (S, nf, npos) that bloch_batch returns, or (nf, npos) for
    every scale, or a scalar (weights >= 0).  Returns a list of (L, grad) per pulse: L = 1/2 sum w_c (m_c - t_c)^2 over the three
    components, the points and the scales, and grad = dL/dRe b1 + i dL/dIm b1, complex (ntime,).  Nothing of point size comes back
    from the device.  Deterministic: a pulse's L and grad bits depend only on the pulse, its grids, targets, weights, m0 and the
    scales.  gr, tp, t1, t2, df, dp and m0 are not differentiated.  magnitude: fit (|Mxy|, mz) instead of (mx, my, mz): targets and weights are then pairs (xy, z)
    per pulse, each entry shaped as before, L = 1/2 sum w_xy (rho - t_xy)^2 + w_z (mz - t_z)^2 with rho = sqrt(mx mx + my my), and
    weights=(w, 0) fits |Mxy| alone; rho = 0 at a point is not an error."""
    who = "bloch_lsq_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    t = _bloch_planes(who, "target", targets, A, magnitude=magnitude)
    T = sum(A.nt)
    loss, grad = np.zeros(A.P), [np.zeros(T) for _ in range(2)]
    m0p = _bloch_m0(A, m0)
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_lsq_mag_batch if magnitude else load_library().mbfir_bloch_lsq_batch
    rc = fn(ctx._h, *A.head, *[_plane(v) for v in m0p], *[_ptr(v) for v in w + t], _ptr(loss), _ptr(grad[0]), _ptr(grad[1]))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _lsq_result([range(n) for n in A.nt], loss, grad)


def bloch_gn_batch(pulses, df, dp, tangents, weights, *, scales=(1.0,), m0=None, magnitude=False, ctx=None):
    """Gauss-Newton products of the fit of bloch_lsq_batch, in one device call (mbfir_bloch_gn_batch): H v = sum_s s J_s' W_s J_s
    (s v) for J = dm / db1 (real-linear in v) and W the weights; arguments as for bloch_lsq_batch, with tangents as bloch_jvp_batch
    takes them: per pulse a complex (n,) direction or K of them of shape (K, n), the same K for every pulse.  Returns per pulse a
    complex (n,) array, or (K, n).  H is symmetric positive semidefinite in the real inner product Re sum conj(u) v.  A product's
    bits depend only on its pulse, grids, weights, direction, m0 and the scales: not on the batch or the direction's place among K.
    magnitude: the products of bloch_lsq_batch(magnitude=True)'s fit, H = J' U' W U J with U the projection on the transverse
    direction u = (mx, my) / rho and on z; weights are then pairs (xy, z) per pulse."""
    who = "bloch_gn_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    rfs = [range(n) for n in A.nt]
    K, keep, vplanes = _tangents(who, tangents, rfs)
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    h = [np.zeros(K * sum(A.nt)) for _ in range(2)]
    m0p = _bloch_m0(A, m0)
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_gn_mag_batch if magnitude else load_library().mbfir_bloch_gn_batch
    rc = fn(ctx._h, *A.head, *[_plane(v) for v in m0p], *[_ptr(v) for v in w], K, *[_ptr(v) for v in vplanes], _ptr(h[0]), _ptr(h[1]))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _gn_result(rfs, K, keep, h)


def bloch_ss_lsq_batch(pulses, df, dp, targets, weights, *, scales=(1.0,), steady=False, magnitude=False, ctx=None):
    """Loss and gradient of a weighted least-squares fit of bloch_batch's steady state (mode 1) in one device call
    (mbfir_bloch_ss_lsq_batch): pulses (each one period), df, dp and scales as for bloch_ss_vjp_batch; targets and
    weights as for bloch_lsq_batch: per pulse a triple (x, y, z) for (mx, my, mz), each entry of the shape (S, nf, npos) that
    bloch_batch(mode=1) returns, or (nf, npos) for every scale, or a scalar (weights >= 0).  Returns a list of (L, grad) per pulse:
    L = 1/2 sum w_c (M_c - t_c)^2 over the three components, the points and the scales, and grad = dL/dRe b1 + i dL/dIm b1, complex
    (ntime,); with steady, a list of (L, grad, (mx, my, mz)), the last being the steady state with bloch_batch(mode=1)'s bits, of
    which the residual is formed.  Without steady nothing of point size comes back from the device.  There is no m0.  Deterministic:
    a pulse's L and grad bits depend only on the pulse, its grids, targets, weights and the scales.  The error grows with
    ||(I - A)^-1||, about T1 / TR.  gr, tp, t1, t2, df and dp are not differentiated.  magnitude: as for bloch_lsq_batch, of the
    steady state: targets and weights are pairs (xy, z) per pulse, and rho is formed of the M that steady returns."""
    who = "bloch_ss_lsq_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    t = _bloch_planes(who, "target", targets, A, magnitude=magnitude)
    T = sum(A.nt)
    loss, grad = np.zeros(P), [np.zeros(T) for _ in range(2)]
    ooff = _offsets([S * f * k for f, k in zip(nf, npos)])
    out = [np.zeros(int(ooff[-1])) for _ in range(3)] if steady else [C.cast(None, _dp)] * 3
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_ss_lsq_mag_batch if magnitude else load_library().mbfir_bloch_ss_lsq_batch
    rc = fn(ctx._h, *A.head, *[_ptr(v) for v in w + t], _ptr(loss), _ptr(grad[0]), _ptr(grad[1]),
            *[_ptr(v) if steady else v for v in out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = _lsq_result([range(n) for n in A.nt], loss, grad)
    if not steady:
        return res
    return [res[q] + (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in out),) for q in range(P)]


def bloch_ss_gn_batch(pulses, df, dp, tangents, weights, *, scales=(1.0,), magnitude=False, ctx=None):
    """Gauss-Newton products of the fit of bloch_ss_lsq_batch, in one device call (mbfir_bloch_ss_gn_batch): H v = sum_s s J_s' W_s
    J_s (s v) for J = dM / db1 of the steady state (real-linear in v) and W the weights; arguments as for bloch_ss_lsq_batch, with
    tangents as bloch_ss_jvp_batch takes them: per pulse a complex (n,) direction or K of them of shape (K, n), the same K for every
    pulse.  Returns per pulse a complex (n,) array, or (K, n).  H is symmetric positive semidefinite in the real inner product Re
    sum conj(u) v.  A product's bits depend only on its pulse, grids, weights, direction and the scales: not on the batch or the
    direction's place among K.  magnitude: the products of bloch_ss_lsq_batch(magnitude=True)'s fit, as for bloch_gn_batch; weights
    are then pairs (xy, z) per pulse."""
    who = "bloch_ss_gn_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    rfs = [range(n) for n in A.nt]
    K, keep, vplanes = _tangents(who, tangents, rfs)
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    h = [np.zeros(K * sum(A.nt)) for _ in range(2)]
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_ss_gn_mag_batch if magnitude else load_library().mbfir_bloch_ss_gn_batch
    rc = fn(ctx._h, *A.head, *[_ptr(v) for v in w], K, *[_ptr(v) for v in vplanes], _ptr(h[0]), _ptr(h[1]))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _gn_result(rfs, K, keep, h)


def _train_echo_planes(who, A, ntr, weights, targets, magnitude=False):
    """The echo term of the train's fused calls.  weights / targets (None: no targets, the products): per pulse a triple whose entries
    are shaped (S, ntr, nf, npos), or (S, nf, npos) / (nf, npos) / a scalar for every repetition -> (ebcast, weight planes, target
    planes): the broadcast form (the planes laid out as the final state's) when no pulse gives a repetition axis.  magnitude: per
    pulse a pair (xy, z) -> the two planes of the magnitude calls."""
    n, form = (2, "pair (xy, z)") if magnitude else (3, "triple (x, y, z)")
    sets = [("weight", weights)] + ([("target", targets)] if targets is not None else [])
    arrs = []
    for what, triples in sets:
        triples = list(triples)
        if len(triples) != A.P:
            raise ValueError("%s: %d %s %ss for %d pulses" % (who, len(triples), what, form.split()[0], A.P))
        per = []
        for q, tri in enumerate(triples):
            if not isinstance(tri, (tuple, list)) or len(tri) != n:
                raise ValueError("%s: the %ss of pulse %d must be a %s" % (who, what, q, form))
            full = (A.S, ntr[q], A.nf[q], A.npos[q])
            short = (A.S, A.nf[q], A.npos[q])
            vs = [np.asarray(v, dtype=np.float64) for v in tri]
            for v in vs:
                if v.shape not in (full, short, short[1:], ()):
                    raise ValueError("%s: a %s of pulse %d has shape %s, not %s, %s, %s or a scalar"
                                     % (who, what, q, v.shape, full, short, short[1:]))
                if what == "weight" and (not np.all(np.isfinite(v)) or np.any(v < 0)):
                    raise ValueError("%s: a weight of pulse %d is negative or not finite" % (who, q))
            per.append(vs)
        arrs.append(per)
    ebcast = not any(v.ndim == 4 for per in arrs for vs in per for v in vs)
    out = []
    for per in arrs:
        planes = [[] for _ in range(n)]
        for q, vs in enumerate(per):
            short = (A.S, A.nf[q], A.npos[q])
            for c, v in enumerate(vs):
                if ebcast:
                    planes[c].append(np.broadcast_to(v, short).ravel())
                else:
                    v = v if v.ndim == 4 else np.broadcast_to(v, short)[:, None]
                    planes[c].append(np.broadcast_to(v, (A.S, ntr[q]) + short[1:]).ravel())
        out.append([_vec(np.concatenate(p)) for p in planes])
    return int(ebcast), out[0], out[1] if targets is not None else None


def _train_rep_weights(who, rep_weights, ntr):
    """rep_weights: None, an array of ntr factors for every pulse, or a Python list of one array per pulse -> None or the table"""
    if rep_weights is None:
        return None
    rw = np.concatenate(_train_tables(who, "rep_weights", rep_weights, ntr, False))
    if not np.all(np.isfinite(rw)) or np.any(rw < 0):
        raise ValueError("%s: a repetition weight is negative or not finite" % who)
    return _vec(rw)


def bloch_train_lsq_batch(pulses, df, dp, ntr, targets, weights, *, rep_weights=None, targets_final=None, weights_final=None,
                          phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, grad_m0=False,
                          magnitude=False, ctx=None):
    """Loss and gradient of a weighted least-squares fit of bloch_train_batch's echoes and final state in one device call
    (mbfir_bloch_train_lsq_batch): pulses, df, dp, ntr, phases, gains, echo, scales, m0, meq and demod as for
    bloch_train_batch.  targets and weights: per pulse a triple (x, y, z) whose entries have the echoes' shape (S, ntr, nf, npos), or
    (S, nf, npos) / (nf, npos) / a scalar for every repetition (weights >= 0); when no pulse gives a repetition axis only point-sized
    planes go up to the device.  Both None: no echo term.  rep_weights: None, or a factor >= 0 per repetition (an array of ntr
    values, or a list of one array per pulse): zeros leave echoes out of the fit.  targets_final / weights_final: None, or per
    pulse a triple as bloch_lsq_batch takes them, for the state after the last repetition.  Returns a list of (L, grad) per pulse,
    L = 1/2 sum_k rw_k sum w_c (echo_kc - t_c)^2 + 1/2 sum wf_c (m_Nc - tf_c)^2 over the components, the points and the scales, and
    grad = dL/dRe b1 + i dL/dIm b1 of the period's samples, complex (ntime,), with bloch_train_vjp_batch's conventions; with
    grad_m0, (L, grad, (gmx, gmy, gmz)), dL/dm0 of shape (S, nf, npos) each.  Nothing echo-sized comes back from the device.
    Deterministic: a pulse's bits depend only on the pulse, its grids, its train, its planes and the scales; targets equal to
    bloch_train_batch's own output give L == 0.0 and a gradient of exact zeros.  magnitude: fit (|Mxy|, mz) of every echo and of the
    final state instead of the vectors (mbfir_bloch_train_lsq_mag_batch): targets, weights, targets_final and
    weights_final are then pairs (xy, z) per pulse, with the shapes a triple's entries may have; rho = sqrt(ex ex + ey ey) has the
    bits of np.sqrt(ex * ex + ey * ey) on bloch_train_batch's output under the same demod, a point with rho == 0 adds
    1/2 rw w_xy t_xy^2 to L and exact zeros to the gradient, and a negative t_xy is taken as it is."""
    who = "bloch_train_lsq_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff = Tn.A, Tn.ntr, Tn.ooff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if (targets is None) != (weights is None):
        raise ValueError("%s: targets and weights are given together or not at all" % who)
    if (targets_final is None) != (weights_final is None):
        raise ValueError("%s: targets_final and weights_final are given together or not at all" % who)
    if targets is None and targets_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, t = (0, [nul] * npl, [nul] * npl) if targets is None else _train_echo_planes(who, A, ntr, weights, targets, magnitude)
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    tf = [nul] * npl if targets_final is None else _bloch_planes(who, "final target", targets_final, A, magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    T = sum(A.nt)
    loss, grad = np.zeros(P), [np.zeros(T) for _ in range(2)]
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_train_lsq_mag_batch if magnitude else load_library().mbfir_bloch_train_lsq_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w + t], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf + tf], _ptr(loss), _ptr(grad[0]), _ptr(grad[1]), *[_plane(v) for v in gm])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    res = _lsq_result([range(n) for n in A.nt], loss, grad)
    if not grad_m0:
        return res
    return [res[q] + (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm),) for q in range(P)]


def bloch_train_gn_batch(pulses, df, dp, ntr, tangents, weights, *, rep_weights=None, weights_final=None, phases=np.pi, gains=1.0,
                         echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, magnitude=False, ctx=None):
    """Gauss-Newton products of the fit of bloch_train_lsq_batch in one device call (mbfir_bloch_train_gn_batch):
    H v = J' W J v for J the Jacobian of (echoes, final state) in the period's b1 (real-linear in v, the scales' and gains' chain
    rule included) and W the weights, rep_weights included; arguments as for bloch_train_lsq_batch without the targets, tangents as
    bloch_train_jvp_batch takes them: per pulse a complex (n,) direction or K of them of shape (K, n), the same K for every pulse.
    weights None: no echo term.  Returns per pulse a complex (n,) array, or (K, n).  H is symmetric positive semidefinite in the real
    inner product Re sum conj(u) v.  A product's bits depend only on its pulse, grids, train, weights, direction and the scales:
    not on the batch, on K or on the direction's place among K.  m0 is not a variable.  magnitude: the products of
    bloch_train_lsq_batch(magnitude=True)'s fit (mbfir_bloch_train_gn_mag_batch), H = J' U' W U J with U the
    projection on the transverse direction of every primal echo and of m_N; weights and weights_final are then pairs (xy, z).  It is
    the Gauss-Newton matrix of the residual (rho - t_xy, e_z - t_z) and drops the curvature of rho across u."""
    who = "bloch_train_gn_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr = Tn.A, Tn.ntr
    if weights is None and weights_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    rfs = [range(n) for n in A.nt]
    K, keep, vplanes = _tangents(who, tangents, rfs)
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, _ = (0, [nul] * npl, None) if weights is None else _train_echo_planes(who, A, ntr, weights, None, magnitude)
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    h = [np.zeros(K * sum(A.nt)) for _ in range(2)]
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_train_gn_mag_batch if magnitude else load_library().mbfir_bloch_train_gn_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf], K, *[_ptr(v) for v in vplanes], _ptr(h[0]), _ptr(h[1]))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _gn_result(rfs, K, keep, h)


def bloch_train_lsq_sched_batch(pulses, df, dp, ntr, targets, weights, *, rep_weights=None, targets_final=None, weights_final=None,
                                phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, grad_gains=True,
                                grad_phases=True, grad_m0=False, magnitude=False, ctx=None):
    """Loss and gradient in the schedule of a weighted least-squares fit of bloch_train_batch's echoes and final state in one device
    call (mbfir_bloch_train_lsq_sched_batch): every argument through demod as for bloch_train_lsq_batch, the loss
    being that call's L.  Returns a list of (L, grad_gains, grad_phases) per pulse: dL/dgains[k] and dL/dphases[k] (per radian) of
    every repetition, float64 of shape (ntr,), summed over the scales and the points, what bloch_train_vjp_sched_batch returns at the
    cotangents rw_k w (echo_k - t) and wf (m_N - tf); None in the place of a half that was not asked for (not both).  With grad_m0 a
    fourth item (gmx, gmy, gmz), dL/dm0 of shape (S, nf, npos).  The gradients are per repetition whatever form the schedule was
    given in (bloch_train_vjp_sched_batch says how a scalar's own derivative follows).  Nothing echo-sized comes back from the
    device, and with point-sized targets and weights nothing echo-sized goes up.  The period is swept once more per (scale,
    distinct gain) for the gains, not at all for the phases.  Deterministic: a pulse's bits depend only on the pulse, its grids, its
    train, its planes and the scales, and a wanted half does not depend on whether the other was asked for; targets equal to
    bloch_train_batch's own output give L == 0.0 and gradients of exact zeros.  magnitude: as for bloch_train_lsq_batch, the fit of
    (|Mxy|, mz) of every echo and of the final state (mbfir_bloch_train_lsq_sched_mag_batch); targets and weights
    are then pairs (xy, z) per pulse."""
    who = "bloch_train_lsq_sched_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr, ooff = Tn.A, Tn.ntr, Tn.ooff
    P, S, nf, npos = A.P, A.S, A.nf, A.npos
    if (targets is None) != (weights is None):
        raise ValueError("%s: targets and weights are given together or not at all" % who)
    if (targets_final is None) != (weights_final is None):
        raise ValueError("%s: targets_final and weights_final are given together or not at all" % who)
    if targets is None and targets_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    if not grad_gains and not grad_phases:
        raise ValueError("%s: neither the gradient in the gains nor the gradient in the phases is wanted" % who)
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, t = (0, [nul] * npl, [nul] * npl) if targets is None else _train_echo_planes(who, A, ntr, weights, targets, magnitude)
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    tf = [nul] * npl if targets_final is None else _bloch_planes(who, "final target", targets_final, A, magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    roff = _offsets(ntr)
    loss = np.zeros(P)
    gg = np.zeros(int(roff[-1])) if grad_gains else None
    gp = np.zeros(int(roff[-1])) if grad_phases else None
    gm = [np.zeros(int(ooff[-1])) for _ in range(3)] if grad_m0 else [nul] * 3
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_train_lsq_sched_mag_batch if magnitude else load_library().mbfir_bloch_train_lsq_sched_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w + t], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf + tf], _ptr(loss), nul if gg is None else _ptr(gg), nul if gp is None else _ptr(gp),
            *[_plane(v) for v in gm])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    cut = lambda v, q: None if v is None else v[roff[q]:roff[q + 1]].copy()
    res = [(float(loss[q]), cut(gg, q), cut(gp, q)) for q in range(P)]
    if not grad_m0:
        return res
    return [res[q] + (tuple(v[ooff[q]:ooff[q + 1]].reshape(S, nf[q], npos[q]) for v in gm),) for q in range(P)]


def bloch_train_gn_sched_batch(pulses, df, dp, ntr, weights, *, tangents_gains=None, tangents_phases=None, rep_weights=None,
                               weights_final=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False,
                               prod_gains=None, prod_phases=None, magnitude=False, ctx=None):
    """Gauss-Newton products of the fit of bloch_train_lsq_sched_batch in one device call (mbfir_bloch_train_gn_sched_batch, DESIGN
    section 8af): H v = J' W J v for J the Jacobian of (echoes, final state) in the schedule (gains, phases) and W the weights,
    rep_weights included; arguments as for bloch_train_lsq_sched_batch without the targets.  tangents_gains / tangents_phases: as
    bloch_train_jvp_sched_batch takes them, None (that half of v is zero; not both) or per pulse a float64 direction of shape (ntr,),
    or K of them of shape (K, ntr), the same K for every pulse and for both; the phases' direction is per radian.  prod_gains /
    prod_phases: which halves of H v are wanted; None = the halves that have directions (not both False).  weights None: no echo
    term.  Returns per pulse (hg, hp), float64 of shape (ntr,) or (K, ntr), None in the place of a half that was not asked for.
    With the 2 ntr unit directions the rows are the dense normal matrix (bloch_train_normal_sched_batch).  H is symmetric positive
    semidefinite.  The period is swept once more per (scale, distinct gain) only when a gains direction or the gains half is asked
    for.  A product's bits depend only on its pulse, grids, train, weights, direction and the scales: not on the batch, on K, on
    the direction's place among K, on whether an all-zero half was passed as None, or on whether the other half was asked for.  m0
    is not a variable.  magnitude: the products of bloch_train_lsq_sched_batch(magnitude=True)'s fit
    (mbfir_bloch_train_gn_sched_mag_batch), as for bloch_train_gn_batch; weights are then pairs (xy, z)."""
    who = "bloch_train_gn_sched_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr = Tn.A, Tn.ntr
    P = A.P
    if weights is None and weights_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    if tangents_gains is None and tangents_phases is None:
        raise ValueError("%s: no direction is given: tangents_gains and tangents_phases are both None" % who)
    K, keep, parts = None, False, []
    for what, v in (("gains", tangents_gains), ("phases", tangents_phases)):
        if v is None:
            parts.append(None)
            continue
        k, kp, d = _train_tangents_sched(who, what, v, ntr)
        if K is not None and (k, kp) != (K, keep):
            raise ValueError("%s: %d directions of the phases for %d of the gains" % (who, k, K))
        K, keep = k, kp
        parts.append(_vec(np.concatenate([x.ravel() for x in d])))
    want_g = tangents_gains is not None if prod_gains is None else bool(prod_gains)
    want_p = tangents_phases is not None if prod_phases is None else bool(prod_phases)
    if not want_g and not want_p:
        raise ValueError("%s: neither the product's gains half nor its phases half is wanted" % who)
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, _ = (0, [nul] * npl, None) if weights is None else _train_echo_planes(who, A, ntr, weights, None, magnitude)
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    roff = _offsets(ntr)
    hg = np.zeros(K * int(roff[-1])) if want_g else None
    hp = np.zeros(K * int(roff[-1])) if want_p else None
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_train_gn_sched_mag_batch if magnitude else load_library().mbfir_bloch_train_gn_sched_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf], K, *[nul if v is None else _ptr(v) for v in parts], nul if hg is None else _ptr(hg),
            nul if hp is None else _ptr(hp))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)

    def cut(v, q):
        if v is None:
            return None
        h = v[K * roff[q]:K * roff[q + 1]].reshape(K, ntr[q]).copy()
        return h if keep else h[0]
    return [(cut(hg, q), cut(hp, q)) for q in range(P)]


def _sched_vary(who, vary):
    """vary -> (gains?, phases?), gains first whatever the order given"""
    vary = (vary,) if isinstance(vary, str) else tuple(vary)
    if not vary or any(v not in ("gains", "phases") for v in vary) or len(set(vary)) != len(vary):
        raise ValueError("%s: vary must name 'gains', 'phases' or both, once each, not %r" % (who, vary))
    return "gains" in vary, "phases" in vary


def bloch_train_normal_sched_batch(pulses, df, dp, ntr, targets, weights, *, vary=("gains", "phases"), rep_weights=None,
                                   targets_final=None, weights_final=None, magnitude=False, **kw):
    """Loss, gradient and dense Gauss-Newton matrix of the fit of bloch_train_lsq_sched_batch in the schedule:
    one bloch_train_lsq_sched_batch call and one bloch_train_gn_sched_batch call with the n unit directions, n = ntr x len(vary), the
    gains first.  The pulses of a call share ntr (an int).  vary: ("gains", "phases"), ("gains",) or ("phases",); without "gains" the
    period's tangent is never launched.  Keywords as bloch_train_lsq_sched_batch's, without the grad_ flags.  Returns per pulse
    (L, g, H): g float64 of length n, H of shape (n, n), row j the product H e_j as the device returned it (symmetric to rounding;
    the caller symmetrises).  magnitude: both calls with magnitude=True, targets and weights pairs (xy, z)."""
    who = "bloch_train_normal_sched_batch"
    for k in ("grad_gains", "grad_phases", "grad_m0", "tangents_gains", "tangents_phases", "prod_gains", "prod_phases"):
        if k in kw:
            raise ValueError("%s: %s is not an argument: vary says which part of the schedule moves" % (who, k))
    vg, vp = _sched_vary(who, vary)
    pulses = list(pulses)
    P = len(pulses)
    n = _train_ints(who, "ntr", ntr, P)
    if P == 0 or any(e != n[0] for e in n):
        raise ValueError("%s: the pulses of a call must share ntr" % who)
    if n[0] < 1:
        raise ValueError("%s: ntr of pulse 0 must be at least 1" % who)
    N = n[0]
    if magnitude:                                         # without it, exactly the calls made before the flag existed
        kw = dict(kw, magnitude=True)
    lsq = bloch_train_lsq_sched_batch(pulses, df, dp, ntr, targets, weights, rep_weights=rep_weights, targets_final=targets_final,
                                      weights_final=weights_final, grad_gains=vg, grad_phases=vp, **kw)
    eye, zero = np.eye(N), np.zeros((N, N))
    dg = [np.concatenate([eye, zero]) if vp else eye] * P if vg else None
    dp_ = [np.concatenate([zero, eye]) if vg else eye] * P if vp else None
    gn = bloch_train_gn_sched_batch(pulses, df, dp, ntr, weights, tangents_gains=dg, tangents_phases=dp_, rep_weights=rep_weights,
                                    weights_final=weights_final, prod_gains=vg, prod_phases=vp, **kw)
    out = []
    for (L, gg, gp), (hg, hp) in zip(lsq, gn):
        out.append((L, np.concatenate([v for v in (gg, gp) if v is not None]), np.concatenate([v for v in (hg, hp) if v is not None], 1)))
    return out


def _rf_g(pulse, q, who, gtype):
    """A pulse of abr_batch / abr2_batch, rf or (rf, g) -> rf and g of dtype gtype, abrm's 2 pi / n per sample where it has none."""
    rf, g = pulse if isinstance(pulse, tuple) else (pulse, None)
    rf = np.asarray(rf, dtype=np.complex128).ravel()
    n = len(rf)
    if n == 0:
        raise ValueError("%s: pulse %d has no samples" % (who, q))
    g = np.full(n, 2.0 * np.pi / n, dtype=gtype) if g is None else np.asarray(g, dtype=gtype).ravel()
    if len(g) != n:
        raise ValueError("%s: g of pulse %d must have one entry per rf sample" % (who, q))
    return rf, g


def _abr_args(who, pulses, x, scales, convention):
    """The checked arguments of abr_batch and abr_vjp_batch: (scales, rf per pulse, g per pulse, grids, points per pulse)."""
    pulses, sc = list(pulses), _vec(scales)
    if not pulses:
        raise ValueError("%s: no pulses" % who)
    if len(sc) == 0:
        raise ValueError("%s: the scale list is empty" % who)
    if convention not in ("abrm", "abr"):
        raise ValueError("%s: convention must be 'abrm' or 'abr'" % who)
    P = len(pulses)
    rfs, gs = zip(*[_rf_g(p, q, who, np.float64) for q, p in enumerate(pulses)])
    xs = [_vec(v) for v in _per_pulse(x, P)]
    if any(len(v) == 0 for v in xs):
        raise ValueError("%s: an empty x" % who)
    nx = [len(xs[0 if len(xs) == 1 else q]) for q in range(P)]
    return sc, rfs, gs, xs, nx


def _plane(o):
    """An argument after `mode` of the batched abr calls: a float64 or int32 array as its pointer; an int, a float or None as it is.
    Shared on purpose by every _abr_call / _abr2_call user: the calls before the lm step pass only arrays and ints, as before."""
    if isinstance(o, np.ndarray):
        return o.ctypes.data_as(_ip) if o.dtype == np.int32 else _ptr(o)
    return o


def _abr_call(fn, ctx, sc, rfs, gs, xs, hard_pulse, planes):
    """mbfir_abr_batch, mbfir_abr_vjp_batch or mbfir_abr_jvp_batch on the checked arguments; planes: what follows `mode` (arrays,
    and the tangent call's ndir)."""
    rf = np.concatenate(rfs)
    rc = fn(ctx._h, len(rfs), _lptr(_offsets([len(r) for r in rfs])), _ptr(_vec(rf.real)), _ptr(_vec(rf.imag)),
            _ptr(_vec(np.concatenate(gs))), len(xs), _lptr(_offsets([len(v) for v in xs])), _ptr(_vec(np.concatenate(xs))), len(sc),
            _ptr(sc), 1 if hard_pulse else 0, *[_plane(o) for o in planes])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)


def abr_batch(pulses, x, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """Many `abrm` / `abr` simulations in one launch (mbfir_abr_batch): every pulse at every scale.  Each pulse is rf (radians per
    sample; 2 pi / n per sample as in abrm) or a tuple (rf, g) with abrm's per-sample g.  x: one array shared by every pulse, or a
    Python list of one array per pulse.  Scale s multiplies rf.  hard_pulse: abrm's hard-pulse model; convention 'abr' returns
    abr.m's b = -conj(b).  Returns a list of (a, b) per pulse, each of shape (S, nx)."""
    sc, rfs, gs, xs, nx = _abr_args("abr_batch", pulses, x, scales, convention)
    P, S = len(rfs), len(sc)
    ooff = _offsets([S * k for k in nx])
    out = [np.zeros(int(ooff[-1])) for _ in range(4)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_batch, ctx, sc, rfs, gs, xs, hard_pulse, out)
    a_all, b_all = out[0] + 1j * out[1], out[2] + 1j * out[3]
    if convention == "abr":
        b_all = -np.conj(b_all)
    return [(a_all[ooff[q]:ooff[q + 1]].reshape(S, nx[q]), b_all[ooff[q]:ooff[q + 1]].reshape(S, nx[q])) for q in range(P)]


def _cotangents(who, cot, shapes, convention):
    """cot: one (ca, cb) per pulse in the shapes the forward call returns -> the four concatenated planes of the C call.  Under
    convention 'abr' the forward call returns -conj(b), so its cotangent maps back as cb -> -conj(cb)."""
    cot = list(cot)
    if len(cot) != len(shapes):
        raise ValueError("%s: %d cotangent pairs for %d pulses" % (who, len(cot), len(shapes)))
    cas, cbs = [], []
    for q, (pair, shape) in enumerate(zip(cot, shapes)):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("%s: the cotangent of pulse %d must be a pair (ca, cb)" % (who, q))
        ca, cb = (np.asarray(v, dtype=np.complex128) for v in pair)
        if ca.shape != shape or cb.shape != shape:
            raise ValueError("%s: the cotangents of pulse %d have shapes %s and %s, the forward call returns %s"
                             % (who, q, ca.shape, cb.shape, shape))
        cas.append(ca.ravel())
        cbs.append(cb.ravel())
    ca, cb = np.concatenate(cas), np.concatenate(cbs)
    if convention == "abr":
        cb = -np.conj(cb)
    return [_vec(ca.real), _vec(ca.imag), _vec(cb.real), _vec(cb.imag)]


def abr_vjp_batch(pulses, x, cot, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The adjoint of abr_batch with respect to rf (mbfir_abr_vjp_batch): pulses, x, scales, hard_pulse and convention as for
    abr_batch; cot: a list of (ca, cb) per pulse, the cotangents of the (a, b) that abr_batch returns, in their shapes (S, nx), with
    ca = dL/dRe a + i dL/dIm a for a real L (torch's convention).  Returns a list of complex (n,) gradients dL/dRe rf + i dL/dIm rf,
    summed over the points and the scales.  Deterministic: a pulse's gradient bits depend only on the pulse, its grid and the
    scales.  g and x are not differentiated."""
    sc, rfs, gs, xs, nx = _abr_args("abr_vjp_batch", pulses, x, scales, convention)
    planes = _cotangents("abr_vjp_batch", cot, [(len(sc), k) for k in nx], convention)
    roff = _offsets([len(r) for r in rfs])
    grad = [np.zeros(int(roff[-1])) for _ in range(2)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_vjp_batch, ctx, sc, rfs, gs, xs, hard_pulse, planes + grad)
    g_all = grad[0] + 1j * grad[1]
    return [g_all[roff[q]:roff[q + 1]] for q in range(len(rfs))]


def abr_vjp_rfg_batch(pulses, x, cot, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The adjoint of abr_batch with respect to rf and to the gradient waveform g (mbfir_abr_vjp_rfg_batch):
    arguments as abr_vjp_batch.  Returns one (grad_rf, grad_g) per pulse: grad_rf as abr_vjp_batch returns it (equal to rounding,
    not to the bit), and grad_g the real (n,) gradient dL/dg, the sum over the points of x times dL/d(x g), summed over the scales
    without a factor (a scale multiplies rf, not g).  A pulse given without g is differentiated at the default 2 pi / n.
    Deterministic as abr_vjp_batch.  x and the scales are not differentiated."""
    sc, rfs, gs, xs, nx = _abr_args("abr_vjp_rfg_batch", pulses, x, scales, convention)
    planes = _cotangents("abr_vjp_rfg_batch", cot, [(len(sc), k) for k in nx], convention)
    roff = _offsets([len(r) for r in rfs])
    grad = [np.zeros(int(roff[-1])) for _ in range(3)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_vjp_rfg_batch, ctx, sc, rfs, gs, xs, hard_pulse, planes + grad)
    g_all = grad[0] + 1j * grad[1]
    return [(g_all[roff[q]:roff[q + 1]], grad[2][roff[q]:roff[q + 1]]) for q in range(len(rfs))]


def _tangents(who, tangents, rfs):
    """tangents: per pulse a complex (n,) or (K, n) array, the same K for every pulse -> (K, whether the K axis is kept, the two
    concatenated planes of the C call: direction-major within a pulse)."""
    tangents = list(tangents)
    if len(tangents) != len(rfs):
        raise ValueError("%s: %d tangents for %d pulses" % (who, len(tangents), len(rfs)))
    vs, lead = [], None
    for q, (t, rf) in enumerate(zip(tangents, rfs)):
        t = np.asarray(t, dtype=np.complex128)
        if t.ndim not in (1, 2) or t.shape[-1] != len(rf) or t.shape[0] == 0:
            raise ValueError("%s: the tangent of pulse %d has shape %s, not (%d,) or (K, %d)" % (who, q, t.shape, len(rf), len(rf)))
        if lead is not None and t.shape[:-1] != lead:
            raise ValueError("%s: the tangent of pulse %d has shape %s where pulse 0 has %s: every pulse takes the same K"
                             % (who, q, t.shape, lead + (len(rfs[0]),)))
        lead = t.shape[:-1]
        vs.append(t.ravel())
    K, keep = (lead[0], True) if lead else (1, False)
    v = np.concatenate(vs)
    return K, keep, [_vec(v.real), _vec(v.imag)]


def _jvp_result(out, tan, ooff, K, keep, shapes, convention):
    """The planes of a tangent call -> [((a, b), (da, db))] per pulse; shapes[q]: (S, nx[, ny])."""
    a_all, b_all = out[0] + 1j * out[1], out[2] + 1j * out[3]
    da_all, db_all = tan[0] + 1j * tan[1], tan[2] + 1j * tan[3]
    if convention == "abr":
        b_all, db_all = -np.conj(b_all), -np.conj(db_all)
    res = []
    for q, shape in enumerate(shapes):
        lo, hi = int(ooff[q]), int(ooff[q + 1])
        tshape = ((K,) if keep else ()) + shape
        res.append(((a_all[lo:hi].reshape(shape), b_all[lo:hi].reshape(shape)),
                    (da_all[K * lo:K * hi].reshape(tshape), db_all[K * lo:K * hi].reshape(tshape))))
    return res


def abr_jvp_batch(pulses, x, tangents, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The tangent of abr_batch with respect to rf (mbfir_abr_jvp_batch): pulses, x, scales, hard_pulse and convention as for
    abr_batch; tangents: per pulse a complex direction of shape (n,), or K of them of shape (K, n), the same K for every pulse.
    Returns a list of ((a, b), (da, db)) per pulse: (a, b) with abr_batch's bits, and (da, db) = d/dt (a, b)(rf + t v) at t = 0 for
    each direction v, of shape (K, S, nx), without the K axis for a 1-D tangent.  Real-linear in v; under convention 'abr' the
    tangent of the returned -conj(b) is -conj(db).  One launch, the directions sharing each sample's trigonometry; a tangent's bits
    depend only on its pulse, scale, point and direction.  g and x are not differentiated."""
    sc, rfs, gs, xs, nx = _abr_args("abr_jvp_batch", pulses, x, scales, convention)
    K, keep, vplanes = _tangents("abr_jvp_batch", tangents, rfs)
    S = len(sc)
    ooff = _offsets([S * k for k in nx])
    out = [np.zeros(int(ooff[-1])) for _ in range(4)]
    tan = [np.zeros(K * int(ooff[-1])) for _ in range(4)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_jvp_batch, ctx, sc, rfs, gs, xs, hard_pulse, [K] + vplanes + out + tan)
    return _jvp_result(out, tan, ooff, K, keep, [(S, k) for k in nx], convention)


def _grids(v, npulse, who, name):
    """One array per pulse (a Python list of arrays, which must then have npulse entries) or one array shared by every pulse."""
    if isinstance(v, list) and len(v) > 0 and all(np.ndim(e) >= 1 for e in v):
        if len(v) != npulse:
            raise ValueError("%s: %s has %d grids for %d pulses" % (who, name, len(v), npulse))
        vs = [_vec(e) for e in v]
    else:
        vs = [_vec(v)]
    if any(len(e) == 0 for e in vs):
        raise ValueError("%s: an empty %s" % (who, name))
    return vs


def _abr2_args(who, pulses, x, y, scales, convention):
    """The checked arguments of abr2_batch and abr2_vjp_batch: (scales, rf per pulse, complex g per pulse, x grids, y grids, nx
    per pulse, ny per pulse)."""
    pulses, sc = list(pulses), _vec(scales)
    if not pulses:
        raise ValueError("%s: no pulses" % who)
    if len(sc) == 0:
        raise ValueError("%s: the scale list is empty" % who)
    if convention not in ("abrm", "abr"):
        raise ValueError("%s: convention must be 'abrm' or 'abr'" % who)
    P = len(pulses)
    rfs, gs = zip(*[_rf_g(p, q, who, np.complex128) for q, p in enumerate(pulses)])
    xs, ys = _grids(x, P, who, "x"), _grids(y, P, who, "y")
    nx = [len(xs[0 if len(xs) == 1 else q]) for q in range(P)]
    ny = [len(ys[0 if len(ys) == 1 else q]) for q in range(P)]
    return sc, rfs, gs, xs, ys, nx, ny


def _abr2_call(fn, ctx, sc, rfs, gs, xs, ys, hard_pulse, planes):
    """mbfir_abr2_batch, mbfir_abr2_vjp_batch or mbfir_abr2_jvp_batch on the checked arguments; planes: what follows `mode` (arrays,
    and the tangent call's ndir)."""
    rf, g = np.concatenate(rfs), np.concatenate(gs)
    rc = fn(ctx._h, len(rfs), _lptr(_offsets([len(r) for r in rfs])), _ptr(_vec(rf.real)), _ptr(_vec(rf.imag)), _ptr(_vec(g.real)),
            _ptr(_vec(g.imag)), len(xs), _lptr(_offsets([len(v) for v in xs])), _ptr(_vec(np.concatenate(xs))), len(ys),
            _lptr(_offsets([len(v) for v in ys])), _ptr(_vec(np.concatenate(ys))), len(sc), _ptr(sc), 1 if hard_pulse else 0,
            *[_plane(o) for o in planes])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)


def abr2_batch(pulses, x, y, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """Many 2D `abrm(rf, g, x, y)` / `abr` simulations in one launch (mbfir_abr2_batch): every pulse at every scale.  Each pulse is
    rf (radians per sample; 2 pi / n per sample along x as in abrm) or a tuple (rf, g) with abrm's complex g (Re g the x gradient,
    Im g the y one).  x and y: each one array shared by every pulse, or a Python list of one array per pulse.  Scale s multiplies
    rf.  hard_pulse: the hard-pulse model (free precession by x Re g + y Im g, then the hard pulse of the sample) that the 2D
    `abrm` does not offer; convention 'abr' returns abr.m's b = -conj(b).  Returns a list of (a, b) per pulse, each of shape
    (S, nx, ny).  Without hard_pulse the bits are those of `abrm(rf * s, g, x, y)`."""
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args("abr2_batch", pulses, x, y, scales, convention)
    P, S = len(rfs), len(sc)
    ooff = _offsets([S * k * j for k, j in zip(nx, ny)])
    out = [np.zeros(int(ooff[-1])) for _ in range(4)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, out)
    a_all, b_all = out[0] + 1j * out[1], out[2] + 1j * out[3]
    if convention == "abr":
        b_all = -np.conj(b_all)
    return [(a_all[ooff[q]:ooff[q + 1]].reshape(S, nx[q], ny[q]), b_all[ooff[q]:ooff[q + 1]].reshape(S, nx[q], ny[q]))
            for q in range(P)]


def abr2_vjp_batch(pulses, x, y, cot, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The adjoint of abr2_batch with respect to rf (mbfir_abr2_vjp_batch): as abr_vjp_batch, with abr2_batch's arguments and the
    cotangents (ca, cb) of each pulse in the shape (S, nx, ny).  Returns a list of complex (n,) gradients; g, x and y are not
    differentiated."""
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args("abr2_vjp_batch", pulses, x, y, scales, convention)
    planes = _cotangents("abr2_vjp_batch", cot, [(len(sc), k, j) for k, j in zip(nx, ny)], convention)
    roff = _offsets([len(r) for r in rfs])
    grad = [np.zeros(int(roff[-1])) for _ in range(2)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_vjp_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, planes + grad)
    g_all = grad[0] + 1j * grad[1]
    return [g_all[roff[q]:roff[q + 1]] for q in range(len(rfs))]


def abr2_vjp_rfg_batch(pulses, x, y, cot, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The adjoint of abr2_batch with respect to rf and to the complex gradient waveform g (mbfir_abr2_vjp_rfg_batch): as
    abr_vjp_rfg_batch, with abr2_vjp_batch's arguments.  grad_g is the complex (n,) dL/dgx + i dL/dgy = dL/dRe g + i dL/dIm g
    (torch's convention for a complex input).  x, y and the scales are not differentiated."""
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args("abr2_vjp_rfg_batch", pulses, x, y, scales, convention)
    planes = _cotangents("abr2_vjp_rfg_batch", cot, [(len(sc), k, j) for k, j in zip(nx, ny)], convention)
    roff = _offsets([len(r) for r in rfs])
    grad = [np.zeros(int(roff[-1])) for _ in range(4)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_vjp_rfg_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, planes + grad)
    g_all, gg_all = grad[0] + 1j * grad[1], grad[2] + 1j * grad[3]
    return [(g_all[roff[q]:roff[q + 1]], gg_all[roff[q]:roff[q + 1]]) for q in range(len(rfs))]


def abr2_jvp_batch(pulses, x, y, tangents, *, scales=(1.0,), hard_pulse=False, convention="abrm", ctx=None):
    """The tangent of abr2_batch with respect to rf (mbfir_abr2_jvp_batch): as abr_jvp_batch, with abr2_batch's arguments; (da, db)
    of each pulse have the shape (K, S, nx, ny), without the K axis for a 1-D tangent.  g, x and y are not differentiated."""
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args("abr2_jvp_batch", pulses, x, y, scales, convention)
    K, keep, vplanes = _tangents("abr2_jvp_batch", tangents, rfs)
    S = len(sc)
    ooff = _offsets([S * k * j for k, j in zip(nx, ny)])
    out = [np.zeros(int(ooff[-1])) for _ in range(4)]
    tan = [np.zeros(K * int(ooff[-1])) for _ in range(4)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_jvp_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, [K] + vplanes + out + tan)
    return _jvp_result(out, tan, ooff, K, keep, [(S, k, j) for k, j in zip(nx, ny)], convention)


# ---- least-squares products of abr_batch / abr2_batch: loss and gradient, Gauss-Newton products (mbfir_abr[2]_lsq / gn_batch) ---
PROFILES = {"ex": 0, "se": 1, "inv": 2, "sat": 2, "st": 3}


def _profile(who, profile):
    if profile not in PROFILES:
        raise ValueError("%s: profile must be one of 'ex', 'se', 'inv' ('sat') or 'st', not %r" % (who, profile))
    return PROFILES[profile]


def _weight_plane(who, weights, shapes):
    """weights: per pulse a real array in the shape the forward call returns, or without its scale axis -> the concatenated plane"""
    weights = list(weights)
    if len(weights) != len(shapes):
        raise ValueError("%s: %d weight arrays for %d pulses" % (who, len(weights), len(shapes)))
    ws = []
    for q, (w, shape) in enumerate(zip(weights, shapes)):
        w = np.asarray(w, dtype=np.float64)
        if w.shape != shape and w.shape != shape[1:]:
            raise ValueError("%s: the weights of pulse %d have shape %s, not %s or %s" % (who, q, w.shape, shape, shape[1:]))
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("%s: a weight of pulse %d is negative or not finite" % (who, q))
        ws.append(np.broadcast_to(w, shape).ravel())
    return _vec(np.concatenate(ws))


def _target_planes(who, targets, shapes, kind):
    targets = list(targets)
    if len(targets) != len(shapes):
        raise ValueError("%s: %d targets for %d pulses" % (who, len(targets), len(shapes)))
    ts = []
    for q, (t, shape) in enumerate(zip(targets, shapes)):
        t = np.asarray(t)
        if t.shape != shape:
            raise ValueError("%s: the target of pulse %d has shape %s, the forward call returns %s" % (who, q, t.shape, shape))
        if kind == 2 and np.iscomplexobj(t) and np.any(t.imag != 0):
            raise ValueError("%s: the profile 'inv' is real, the target of pulse %d is complex" % (who, q))
        ts.append(t.astype(np.complex128).ravel())
    t = np.concatenate(ts)
    return [_vec(t.real), _vec(t.imag)]


def _lsq_result(rfs, loss, grad):
    roff = _offsets([len(r) for r in rfs])
    g_all = grad[0] + 1j * grad[1]
    return [(float(loss[q]), g_all[roff[q]:roff[q + 1]]) for q in range(len(rfs))]


def _gn_result(rfs, K, keep, h):
    roff = _offsets([len(r) for r in rfs])
    h_all = h[0] + 1j * h[1]
    return [h_all[K * roff[q]:K * roff[q + 1]].reshape((K, len(rfs[q])) if keep else (len(rfs[q]),)) for q in range(len(rfs))]


def abr_lsq_batch(pulses, x, targets, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
    """Loss and gradient of a weighted least-squares fit of abr_batch's profile, in one device call (mbfir_abr_lsq_batch): pulses,
    x, scales and hard_pulse as for abr_batch, in the 'abrm' convention only (the profiles are those of ab2ex, ab2se, ab2inv /
    ab2sat and ab2st on abrm's (a, b)).  profile: 'ex' f = 2 conj(a) b, 'se' f = i b^2, 'inv' (alias 'sat') f = 1 - 2 |b|^2, 'st'
    f = i a^2.  targets: per pulse an array of the shape (S, nx) that abr_batch returns (real for 'inv'); weights: per pulse a real
    array >= 0 of that shape, or of shape (nx,) for every scale.  Returns a list of (L, grad) per pulse: L = 1/2 sum w |f - t|^2
    over the points and scales, and grad = dL/dRe rf + i dL/dIm rf, complex (n,).  Nothing of point size comes back from the
    device.  Deterministic: a pulse's L and grad bits depend only on the pulse, its grid, target, weights and the scales."""
    who = "abr_lsq_batch"
    sc, rfs, gs, xs, nx = _abr_args(who, pulses, x, scales, "abrm")
    kind = _profile(who, profile)
    shapes = [(len(sc), k) for k in nx]
    planes = [kind, _weight_plane(who, weights, shapes)] + _target_planes(who, targets, shapes, kind)
    R = sum(len(r) for r in rfs)
    loss, grad = np.zeros(len(rfs)), [np.zeros(R) for _ in range(2)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_lsq_batch, ctx, sc, rfs, gs, xs, hard_pulse, planes + [loss] + grad)
    return _lsq_result(rfs, loss, grad)


def abr2_lsq_batch(pulses, x, y, targets, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
    """abr_lsq_batch for abr2_batch (mbfir_abr2_lsq_batch): targets of shape (S, nx, ny), weights of that shape or (nx, ny)."""
    who = "abr2_lsq_batch"
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args(who, pulses, x, y, scales, "abrm")
    kind = _profile(who, profile)
    shapes = [(len(sc), k, j) for k, j in zip(nx, ny)]
    planes = [kind, _weight_plane(who, weights, shapes)] + _target_planes(who, targets, shapes, kind)
    R = sum(len(r) for r in rfs)
    loss, grad = np.zeros(len(rfs)), [np.zeros(R) for _ in range(2)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_lsq_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, planes + [loss] + grad)
    return _lsq_result(rfs, loss, grad)


def abr_gn_batch(pulses, x, tangents, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
    """Gauss-Newton products of the fit of abr_lsq_batch, in one device call (mbfir_abr_gn_batch): H v = J^H W J v for J = df / drf
    (real-linear in v) and W the weights; arguments as for abr_lsq_batch ('abrm' convention only), with tangents as abr_jvp_batch
    takes them: per pulse a complex (n,) direction or K of them of shape (K, n), the same K for every pulse.  Returns per pulse a
    complex (n,) array, or (K, n).  H is symmetric positive semidefinite in the real inner product Re sum conj(u) v.  A product's
    bits depend only on its pulse, grid, weights, direction and the scales: not on the batch or the direction's place among K."""
    who = "abr_gn_batch"
    sc, rfs, gs, xs, nx = _abr_args(who, pulses, x, scales, "abrm")
    kind = _profile(who, profile)
    K, keep, vplanes = _tangents(who, tangents, rfs)
    w = _weight_plane(who, weights, [(len(sc), k) for k in nx])
    h = [np.zeros(K * sum(len(r) for r in rfs)) for _ in range(2)]
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_gn_batch, ctx, sc, rfs, gs, xs, hard_pulse, [kind, w, K] + vplanes + h)
    return _gn_result(rfs, K, keep, h)


def abr2_gn_batch(pulses, x, y, tangents, weights, *, profile="ex", scales=(1.0,), hard_pulse=False, ctx=None):
    """abr_gn_batch for abr2_batch (mbfir_abr2_gn_batch): weights of shape (S, nx, ny) or (nx, ny)."""
    who = "abr2_gn_batch"
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args(who, pulses, x, y, scales, "abrm")
    kind = _profile(who, profile)
    K, keep, vplanes = _tangents(who, tangents, rfs)
    w = _weight_plane(who, weights, [(len(sc), k, j) for k, j in zip(nx, ny)])
    h = [np.zeros(K * sum(len(r) for r in rfs)) for _ in range(2)]
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_gn_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, [kind, w, K] + vplanes + h)
    return _gn_result(rfs, K, keep, h)


# ---- the Levenberg-Marquardt step solved on the device (mbfir_abr[2]_lm_step_batch) --------------------------------------------------
LM_STATUS = ("rtol", "cg", "breakdown")


def _lm_args(who, rfs, rhs, mu, cg, rtol):
    """The checked right-hand sides, dampings, cap and tolerance -> (the two planes of rhs, mu per pulse, cg, rtol)."""
    rhs = list(rhs)
    if len(rhs) != len(rfs):
        raise ValueError("%s: %d right-hand sides for %d pulses" % (who, len(rhs), len(rfs)))
    bs = []
    for q, (b, rf) in enumerate(zip(rhs, rfs)):
        b = np.asarray(b, dtype=np.complex128)
        if b.shape != (len(rf),):
            raise ValueError("%s: the right-hand side of pulse %d has shape %s, not (%d,)" % (who, q, b.shape, len(rf)))
        bs.append(b)
    try:
        m = _vec(np.broadcast_to(np.asarray(mu, dtype=np.float64), (len(rfs),)))
    except ValueError:
        raise ValueError("%s: mu must be a number or one number per pulse" % who) from None
    if not np.all(np.isfinite(m)) or np.any(m < 0):
        raise ValueError("%s: a damping mu is negative or not finite" % who)
    if int(cg) != cg or cg < 0:
        raise ValueError("%s: cg must be an integer, at least 0" % who)
    if not rtol >= 0:
        raise ValueError("%s: rtol is negative or not a number" % who)
    b = np.concatenate(bs)
    return [_vec(b.real), _vec(b.imag)], m, int(cg), float(rtol)


def _lm_planes(who, kind, w, bplanes, m, cg, rtol, targets, shapes, rfs):
    """What follows `mode` in the C call, and the output arrays: d (2), ncg, rr, gg, status, and with targets loss, grad (2)."""
    P, R = len(rfs), sum(len(r) for r in rfs)
    tplanes = [None, None] if targets is None else _target_planes(who, targets, shapes, kind)
    out = [np.zeros(R), np.zeros(R), np.zeros(P, dtype=np.int32), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)]
    out += [None, None, None] if targets is None else [np.zeros(P), np.zeros(R), np.zeros(R)]
    return [kind, w] + bplanes + [m, cg, C.c_double(rtol)] + tplanes + out, out


def _lm_result(rfs, out):
    roff = _offsets([len(r) for r in rfs])
    d_all = out[0] + 1j * out[1]
    res = []
    for q in range(len(rfs)):
        lo, hi = int(roff[q]), int(roff[q + 1])
        info = dict(ncg=int(out[2][q]), rr=float(out[3][q]), gg=float(out[4][q]), status=LM_STATUS[int(out[5][q])])
        if out[6] is not None:
            info["loss"] = float(out[6][q])
            info["grad"] = out[7][lo:hi] + 1j * out[8][lo:hi]
        res.append((d_all[lo:hi], info))
    return res


def abr_lm_step_batch(pulses, x, rhs, weights, mu, *, targets=None, cg=8, rtol=1e-6, profile="ex", scales=(1.0,), hard_pulse=False,
                      ctx=None):
    """One damped Gauss-Newton (Levenberg-Marquardt) step per pulse, solved on the device in one call (mbfir_abr_lm_step_batch):
    conjugate gradients on (H + mu I) d = rhs from d = 0, H = J^H W J as abr_gn_batch applies it, in the inner product
    <u, v> = sum Re(conj(u) v); at most cg iterations, while <r, r> > rtol <rhs, rhs>.  pulses, x, weights, profile, scales and
    hard_pulse as for abr_gn_batch; rhs: per pulse a complex (n,) array; mu: a number >= 0 or one per pulse.  With targets (as for
    abr_lsq_batch) the loss and gradient at rf + d come back too.  Returns a list of (d, info) per pulse: info holds 'ncg' (iterations
    done), 'rr' (the last <r, r>), 'gg' (<rhs, rhs>) and 'status': 'rtol' (tolerance reached), 'cg' (the cap reached) or 'breakdown'
    (<p, (H + mu) p> not finite or not > 0: d is the one before that iteration); with targets also 'loss' and 'grad', with the
    bits of abr_lsq_batch at rf + d.  The host reads nothing between the iterations, so cg is also a launch count: all 2 cg
    launches are queued, those of pulses that have stopped returning at once; keep cg at the iterations a step is worth.  Deterministic: a pulse's results depend only
    on the pulse, its grid, weights, target, rhs, mu, cg, rtol and the scales, not on the batch or when its neighbours stop."""
    who = "abr_lm_step_batch"
    sc, rfs, gs, xs, nx = _abr_args(who, pulses, x, scales, "abrm")
    kind = _profile(who, profile)
    shapes = [(len(sc), k) for k in nx]
    bplanes, m, cg, rtol = _lm_args(who, rfs, rhs, mu, cg, rtol)
    planes, out = _lm_planes(who, kind, _weight_plane(who, weights, shapes), bplanes, m, cg, rtol, targets, shapes, rfs)
    ctx = ctx or get_context()
    _abr_call(load_library().mbfir_abr_lm_step_batch, ctx, sc, rfs, gs, xs, hard_pulse, planes)
    return _lm_result(rfs, out)


def abr2_lm_step_batch(pulses, x, y, rhs, weights, mu, *, targets=None, cg=8, rtol=1e-6, profile="ex", scales=(1.0,),
                       hard_pulse=False, ctx=None):
    """abr_lm_step_batch for abr2_batch (mbfir_abr2_lm_step_batch): weights and targets as for abr2_gn_batch / abr2_lsq_batch."""
    who = "abr2_lm_step_batch"
    sc, rfs, gs, xs, ys, nx, ny = _abr2_args(who, pulses, x, y, scales, "abrm")
    kind = _profile(who, profile)
    shapes = [(len(sc), k, j) for k, j in zip(nx, ny)]
    bplanes, m, cg, rtol = _lm_args(who, rfs, rhs, mu, cg, rtol)
    planes, out = _lm_planes(who, kind, _weight_plane(who, weights, shapes), bplanes, m, cg, rtol, targets, shapes, rfs)
    ctx = ctx or get_context()
    _abr2_call(load_library().mbfir_abr2_lm_step_batch, ctx, sc, rfs, gs, xs, ys, hard_pulse, planes)
    return _lm_result(rfs, out)


def bloch_lm_step_batch(pulses, df, dp, rhs, weights, mu, *, targets=None, cg=8, rtol=1e-6, scales=(1.0,), m0=None, magnitude=False,
                        ctx=None):
    """abr_lm_step_batch for bloch_batch's model, relaxation included (mbfir_bloch_lm_step_batch): conjugate
    gradients on (H + mu I) d = rhs from d = 0, H = sum_s s J_s' W_s J_s (s .) as bloch_gn_batch applies it, solved on the device in
    one call.  pulses, df, dp, weights, scales and m0 as for bloch_gn_batch; rhs: per pulse a complex (n,) array; mu: a number >= 0
    or one per pulse; cg and rtol as for abr_lm_step_batch.  With targets (as for bloch_lsq_batch) the loss and gradient at b1 + d
    come back too, with the bits of bloch_lsq_batch there.  Returns a list of (d, info) per pulse: info holds 'ncg', 'rr', 'gg' and
    'status' ('rtol', 'cg' or 'breakdown'), and with targets 'loss' and 'grad'.  The host reads nothing between the iterations, so
    cg is also a launch count.  Deterministic: a pulse's results depend only on the pulse, its grids, weights, targets, m0, rhs, mu,
    cg, rtol and the scales, not on the batch or when its neighbours stop.  magnitude: the step of the magnitude fit (DESIGN section
    8ah): H as bloch_gn_batch(magnitude=True) applies it, the trial's loss and gradient with the bits of
    bloch_lsq_batch(magnitude=True); weights and targets are then pairs (xy, z) per pulse."""
    who = "bloch_lm_step_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    rfs = [range(n) for n in A.nt]
    bplanes, m, cg, rtol = _lm_args(who, rfs, rhs, mu, cg, rtol)
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    t = [None] * len(w) if targets is None else _bloch_planes(who, "target", targets, A, magnitude=magnitude)
    P, T = A.P, sum(A.nt)
    out = [np.zeros(T), np.zeros(T), np.zeros(P, dtype=np.int32), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)]
    out += [None, None, None] if targets is None else [np.zeros(P), np.zeros(T), np.zeros(T)]
    m0p = _bloch_m0(A, m0)
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_lm_step_mag_batch if magnitude else load_library().mbfir_bloch_lm_step_batch
    rc = fn(ctx._h, *A.head, *[_plane(v) for v in m0p], *[_ptr(v) for v in w + bplanes], _ptr(m), cg, C.c_double(rtol),
            *[_plane(v) for v in t + out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _lm_result(rfs, out)


def bloch_ss_lm_step_batch(pulses, df, dp, rhs, weights, mu, *, targets=None, cg=8, rtol=1e-6, scales=(1.0,), magnitude=False, ctx=None):
    """bloch_lm_step_batch for the steady state of the period, bloch_batch's mode 1 (mbfir_bloch_ss_lm_step_batch, DESIGN section
    8v): conjugate gradients on (H + mu I) d = rhs from d = 0, H = sum_s s J_s' W_s J_s (s .) as bloch_ss_gn_batch applies it, solved
    on the device in one call.  pulses (each one period), df, dp, weights and scales as for bloch_ss_gn_batch; rhs: per pulse a
    complex (n,) array; mu: a number >= 0 or one per pulse; cg and rtol as for abr_lm_step_batch.  With targets (as for
    bloch_ss_lsq_batch) the loss and gradient at b1 + d come back too, with the bits of bloch_ss_lsq_batch there.  Returns a list of
    (d, info) per pulse: info holds 'ncg', 'rr', 'gg' and 'status' ('rtol', 'cg' or 'breakdown'), and with targets 'loss' and 'grad'.
    There is no m0.  b1 is fixed within the solve, so (I - A)^-1 and the steady state are computed once per call.  The host reads
    nothing between the iterations, so cg is also a launch count.  Deterministic: a pulse's results depend only on the pulse, its
    grids, weights, targets, rhs, mu, cg, rtol and the scales, not on the batch or when its neighbours stop.  magnitude: as for
    bloch_lm_step_batch, on bloch_ss_gn_batch(magnitude=True) and bloch_ss_lsq_batch(magnitude=True)."""
    who = "bloch_ss_lm_step_batch"
    A = _BlochArgs(who, pulses, df, dp, scales)
    rfs = [range(n) for n in A.nt]
    bplanes, m, cg, rtol = _lm_args(who, rfs, rhs, mu, cg, rtol)
    w = _bloch_planes(who, "weight", weights, A, weights=True, magnitude=magnitude)
    t = [None] * len(w) if targets is None else _bloch_planes(who, "target", targets, A, magnitude=magnitude)
    P, T = A.P, sum(A.nt)
    out = [np.zeros(T), np.zeros(T), np.zeros(P, dtype=np.int32), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)]
    out += [None, None, None] if targets is None else [np.zeros(P), np.zeros(T), np.zeros(T)]
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_ss_lm_step_mag_batch if magnitude else load_library().mbfir_bloch_ss_lm_step_batch
    rc = fn(ctx._h, *A.head, *[_ptr(v) for v in w + bplanes], _ptr(m), cg, C.c_double(rtol), *[_plane(v) for v in t + out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _lm_result(rfs, out)


def bloch_train_lm_step_batch(pulses, df, dp, ntr, rhs, weights, mu, *, targets=None, rep_weights=None, targets_final=None,
                              weights_final=None, phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, cg=8,
                              rtol=1e-6, magnitude=False, ctx=None):
    """bloch_lm_step_batch for the echoes of a pulse train, bloch_train_batch's model (mbfir_bloch_train_lm_step_batch, DESIGN section
    8ac): conjugate gradients on (H + mu I) d = rhs from d = 0, H = J' W J as bloch_train_gn_batch applies it (echo term, rep_weights,
    final term, the scales' and gains' chain rule), solved on the device in one call.  pulses (each one period), df, dp, ntr,
    weights, rep_weights, weights_final, phases, gains, echo, scales, m0, meq and demod as for bloch_train_gn_batch; rhs: per pulse a
    complex (n,) array; mu: a number >= 0 or one per pulse; cg and rtol as for abr_lm_step_batch.  With targets and / or
    targets_final (as for bloch_train_lsq_batch: one for every term that has weights) the loss and gradient at b1 + d come back too,
    with the bits of bloch_train_lsq_batch there.  Returns a list of (d, info) per pulse: info holds 'ncg', 'rr', 'gg' and 'status'
    ('rtol', 'cg' or 'breakdown'), and with targets 'loss' and 'grad'.  b1 is fixed within the solve, so the propagators' planes
    and the checkpoints of the period's adjoint are computed once per call.  The host reads nothing between the iterations, so cg is
    also a launch count.  Deterministic: a pulse's results depend only on the pulse, its grids, its train, weights, targets, m0, rhs,
    mu, cg, rtol and the scales, not on the batch or when its neighbours stop.  magnitude: the step of the magnitude fit
    (mbfir_bloch_train_lm_step_mag_batch): H as bloch_train_gn_batch(magnitude=True) applies it, the trial's loss
    and gradient with the bits of bloch_train_lsq_batch(magnitude=True); weights and targets are then pairs (xy, z) per pulse."""
    who = "bloch_train_lm_step_batch"
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr = Tn.A, Tn.ntr
    if weights is None and weights_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    if targets is not None and weights is None:
        raise ValueError("%s: targets are given for an echo term that has no weights" % who)
    if targets_final is not None and weights_final is None:
        raise ValueError("%s: targets_final are given for a final term that has no weights" % who)
    trial = targets is not None or targets_final is not None
    if trial and ((weights is not None and targets is None) or (weights_final is not None and targets_final is None)):
        raise ValueError("%s: with targets, every term that has weights needs its own" % who)
    rfs = [range(n) for n in A.nt]
    bplanes, m, cg, rtol = _lm_args(who, rfs, rhs, mu, cg, rtol)
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, t = (0, [nul] * npl, None) if weights is None else _train_echo_planes(who, A, ntr, weights, targets, magnitude)
    t = [nul] * npl if t is None else t
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    tf = [nul] * npl if targets_final is None else _bloch_planes(who, "final target", targets_final, A, magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    P, T = A.P, sum(A.nt)
    out = [np.zeros(T), np.zeros(T), np.zeros(P, dtype=np.int32), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)]
    out += [np.zeros(P), np.zeros(T), np.zeros(T)] if trial else [None, None, None]
    ctx = ctx or get_context()
    fn = load_library().mbfir_bloch_train_lm_step_mag_batch if magnitude else load_library().mbfir_bloch_train_lm_step_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf], *[_ptr(v) for v in bplanes], _ptr(m), cg, C.c_double(rtol), *[_plane(v) for v in t + tf + out])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    return _lm_result(rfs, out)


def bloch_train_lm_step_sched_batch(pulses, df, dp, ntr, weights, mu, *, vary=("gains", "phases"), b=None, targets=None,
                                    targets_final=None, cg=8, rtol=1e-6, rep_weights=None, weights_final=None, phases=np.pi, gains=1.0,
                                    echo=None, scales=(1.0,), m0=None, meq=1.0, demod=False, magnitude=False, ctx=None):
    """The Levenberg-Marquardt step of a train's schedule, the gain and the RF phase of every repetition, evaluated and solved at the
    same schedule in one device call (mbfir_bloch_train_lm_step_sched_batch), so that the propagators of a
    schedule are swept once for both.  pulses, df, dp, ntr, weights, rep_weights, weights_final, phases, gains, echo, scales, m0, meq
    and demod as for bloch_train_gn_sched_batch.  With targets and / or targets_final (as for bloch_train_lsq_sched_batch: one for
    every term that has weights) the loss and the gradient at the call's schedule come back with the bits of
    bloch_train_lsq_sched_batch.  Then conjugate gradients on (H + mu I) d = b from d = 0, H = J' W J restricted to the halves vary
    names (("gains", "phases"), ("gains",) or ("phases",)), as bloch_train_gn_sched_batch applies it at that schedule; mu: a number
    >= 0 or one per pulse; cg and rtol as for abr_lm_step_batch; cg = 0 evaluates only.  b: None (with targets: the negated gradient,
    which never leaves the device) or per pulse a pair (b_gains, b_phases) of float64 (ntr,) arrays, None in the place of a half that
    does not vary.  There is no trial at schedule + d: a trial has other gains, so its own sweeps; evaluate it with the next call,
    which solves the next step too.  Returns a list of (d_gains, d_phases, info) per pulse, None for a half not varied; info holds
    'ncg', 'rr', 'gg' and 'status' ('rtol', 'cg' or 'breakdown'), and with targets 'loss', 'grad_gains' and 'grad_phases' (None for a
    half not varied).  Without "gains" in vary the period's tangent is never launched.  Deterministic: a pulse's results depend only
    on the pulse, its grids, its train, weights, targets, m0, b, mu, cg, rtol and the scales, not on the batch or when its neighbours
    stop.  magnitude: the step of the magnitude fit (mbfir_bloch_train_lm_step_sched_mag_batch): the evaluation
    with the bits of bloch_train_lsq_sched_batch(magnitude=True), H as bloch_train_gn_sched_batch(magnitude=True) applies it; weights
    and targets are then pairs (xy, z) per pulse."""
    who = "bloch_train_lm_step_sched_batch"
    vg, vp = _sched_vary(who, vary)
    Tn = _TrainArgs(who, pulses, df, dp, ntr, phases, gains, echo, scales, meq, demod)
    A, ntr = Tn.A, Tn.ntr
    P = A.P
    if weights is None and weights_final is None:
        raise ValueError("%s: neither an echo term nor a final term is given" % who)
    if targets is not None and weights is None:
        raise ValueError("%s: targets are given for an echo term that has no weights" % who)
    if targets_final is not None and weights_final is None:
        raise ValueError("%s: targets_final are given for a final term that has no weights" % who)
    evalu = targets is not None or targets_final is not None
    if evalu and ((weights is not None and targets is None) or (weights_final is not None and targets_final is None)):
        raise ValueError("%s: with targets, every term that has weights needs its own" % who)
    if not evalu and b is None:
        raise ValueError("%s: neither targets nor a right-hand side b is given" % who)
    try:
        m = _vec(np.broadcast_to(np.asarray(mu, dtype=np.float64), (P,)))
    except ValueError:
        raise ValueError("%s: mu must be a number or one number per pulse" % who) from None
    if not np.all(np.isfinite(m)) or np.any(m < 0):
        raise ValueError("%s: a damping mu is negative or not finite" % who)
    if int(cg) != cg or cg < 0:
        raise ValueError("%s: cg must be an integer, at least 0" % who)
    if not rtol >= 0:
        raise ValueError("%s: rtol is negative or not a number" % who)
    bplanes = [None, None]
    if b is not None:
        b = list(b)
        if len(b) != P:
            raise ValueError("%s: %d right-hand sides for %d pulses" % (who, len(b), P))
        halves = [[], []]
        for q, pair in enumerate(b):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("%s: the right-hand side of pulse %d must be a pair (b_gains, b_phases)" % (who, q))
            for i, (name, on) in enumerate((("gains", vg), ("phases", vp))):
                if (pair[i] is not None) != on:
                    raise ValueError("%s: the right-hand side of pulse %d has %s for the %s, which %s" %
                                     (who, q, "a half" if not on else "None", name, "vary" if on else "do not vary"))
                if on:
                    v = np.asarray(pair[i], dtype=np.float64)
                    if v.shape != (ntr[q],):
                        raise ValueError("%s: the %s half of the right-hand side of pulse %d has shape %s, not (%d,)" %
                                         (who, name, q, v.shape, ntr[q]))
                    halves[i].append(v)
        bplanes = [_vec(np.concatenate(h)) if on else None for h, on in zip(halves, (vg, vp))]
    nul = C.cast(None, _dp)
    npl = 2 if magnitude else 3
    eb, w, t = (0, [nul] * npl, None) if weights is None else _train_echo_planes(who, A, ntr, weights, targets, magnitude)
    t = [nul] * npl if t is None else t
    wf = [nul] * npl if weights_final is None else _bloch_planes(who, "final weight", weights_final, A, weights=True,
                                                                 magnitude=magnitude)
    tf = [nul] * npl if targets_final is None else _bloch_planes(who, "final target", targets_final, A, magnitude=magnitude)
    rw = _train_rep_weights(who, rep_weights, ntr)
    m0p = _bloch_m0(A, m0)
    roff = _offsets(ntr)
    R = int(roff[-1])
    d = [np.zeros(R) if on else None for on in (vg, vp)]
    st = [np.zeros(P, dtype=np.int32), np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)]
    loss = np.zeros(P) if evalu else None
    g = [np.zeros(R) if on and evalu else None for on in (vg, vp)]
    ctx = ctx or get_context()
    lib = load_library()
    fn = lib.mbfir_bloch_train_lm_step_sched_mag_batch if magnitude else lib.mbfir_bloch_train_lm_step_sched_batch
    rc = fn(ctx._h, *A.head, *Tn.tail, *[_plane(v) for v in m0p], eb, *[_plane(v) for v in w + t], _plane(nul if rw is None else rw),
            *[_plane(v) for v in wf + tf], *[_plane(nul if v is None else v) for v in bplanes], _ptr(m), int(cg),
            C.c_double(float(rtol)), *[_plane(nul if v is None else v) for v in d + st + [loss] + g])
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    cut = lambda v, q: None if v is None else v[roff[q]:roff[q + 1]].copy()
    res = []
    for q in range(P):
        info = dict(ncg=int(st[0][q]), rr=float(st[1][q]), gg=float(st[2][q]), status=LM_STATUS[int(st[3][q])])
        if evalu:
            info.update(loss=float(loss[q]), grad_gains=cut(g[0], q), grad_phases=cut(g[1], q))
        res.append((cut(d[0], q), cut(d[1], q), info))
    return res


from .refine import (refine_batch, refine_bloch_batch, refine_bloch_ss_batch, refine_bloch_train_batch,   # noqa: E402  (batched
                     refine_bloch_train_lm_batch, refine_bloch_train_sched_batch,                          # Levenberg-Marquardt on the calls above)
                     refine_bloch_train_sched_lm_batch)


def jvp_group():
    """The directions one workgroup of abr_jvp_batch / abr2_jvp_batch carries (mbfir_test_jvp_group)."""
    return int(load_library().mbfir_test_jvp_group())


def bloch_ss_jvp_group():
    """The directions one workgroup of bloch_ss_jvp_batch carries (mbfir_test_bloch_ss_jvp_group)."""
    return int(load_library().mbfir_test_bloch_ss_jvp_group())


def bloch_jvp_group():
    """The directions one workgroup of bloch_jvp_batch carries (mbfir_test_bloch_jvp_group)."""
    return int(load_library().mbfir_test_bloch_jvp_group())


def bloch_train_jvp_group():
    """The directions one workgroup of bloch_train_jvp_batch carries (mbfir_test_bloch_train_jvp_group): (in the period's kernel, in
    the repetitions' kernel)."""
    lib = load_library()
    return int(lib.mbfir_test_bloch_train_jvp_group(0)), int(lib.mbfir_test_bloch_train_jvp_group(1))


def bloch_train_sched_jvp_group():
    """The directions one workgroup of bloch_train_jvp_sched_batch carries (mbfir_test_bloch_train_sched_jvp_group)."""
    return int(load_library().mbfir_test_bloch_train_sched_jvp_group())


def test_ddsolve(H, U, X, bh, bl, ctx=None, factor=False):
    """(H + U' diag(X) U)^-1 b through the device's double-double kernels; b, x: (nrhs, n) hi / lo parts.
    factor=True also returns the Cholesky factor (hi, lo)."""
    ctx = ctx or get_context()
    H = np.ascontiguousarray(H, dtype=np.float64)
    U = np.ascontiguousarray(U, dtype=np.float64).reshape(-1, H.shape[0])
    X = _vec(X)
    bh = np.ascontiguousarray(np.atleast_2d(bh), dtype=np.float64)
    bl = np.ascontiguousarray(np.atleast_2d(bl), dtype=np.float64)
    xh, xl = np.zeros_like(bh), np.zeros_like(bh)
    nfix = C.c_int(0)
    Lh, Ll = (np.zeros_like(H), np.zeros_like(H)) if factor else (None, None)
    _check(ctx, load_library().mbfir_test_ddsolve(ctx._h, H.shape[0], U.shape[0], _ptr(H), _ptr(U), _ptr(X), bh.shape[0],
                                                  _ptr(bh), _ptr(bl), _ptr(xh), _ptr(xl), C.byref(nfix),
                                                  _ptr(Lh) if factor else None, _ptr(Ll) if factor else None))
    if factor:
        return xh, xl, nfix.value, np.tril(Lh), np.tril(Ll)
    return xh, xl, nfix.value


DD_FORMS = {"single": 0, "mw": 1, "bi": 2}          # k_dd_trsv, k_dd_trsv_mw, k_dd_trsv_bi
DD_SYNC_LOST = 1 << 20                              # what a lost hand-off adds to the pivot counter (dev_common.h)
DDSTAGES_OUT = ("Hh", "Hl", "d0", "Lh", "Ll", "Lth", "Ltl", "ri", "dinv", "xh", "xl")


def test_ddstages(H, U, X, bh, bl, *, pivtol=1e-28, form="mw", nsolve=1, sentinel=np.nan, ctx=None):
    """The double-double kernels of ddlin.hip stage by stage (mbfir_test_ddstages): the rank-k update H + U' diag(X) U, the blocked
    Cholesky factorisation (for form 'bi' with the inverses of the 64 x 64 diagonal blocks) and `nsolve` solves of b (nrhs x n, hi / lo)
    by the kernel `form` names ('single' | 'mw' | 'bi') on one flag array, epochs 1 .. nsolve.  Returns a dict, everything at the
    padded size np = n rounded up to 64 and pre-filled with `sentinel` where a kernel is to write: Hh, Hl (np, np) after the update;
    d0 (np); Lh, Ll (np, np) the same buffers after the factorisation; Lth, Ltl (np, np); ri (2, np); dinv (2, np / 64, 64, 64);
    xh, xl (nsolve, 2, np); counter (2: after the factorisation, after the solves).  The arguments are checked by the library: a
    bad one raises ValueError with its message."""
    ctx = ctx or get_context()
    H = np.ascontiguousarray(H, dtype=np.float64)
    n = int(H.shape[0])
    U = np.ascontiguousarray(U, dtype=np.float64).reshape(-1, n)
    X = _vec(X)
    bh = np.ascontiguousarray(np.atleast_2d(bh), dtype=np.float64)
    bl = np.ascontiguousarray(np.atleast_2d(bl), dtype=np.float64)
    if form not in DD_FORMS:
        raise ValueError("form must be one of %s" % (sorted(DD_FORMS),))
    npd, ns = -(-n // 64) * 64, max(int(nsolve), 1)
    shapes = dict(Hh=(npd, npd), Hl=(npd, npd), d0=(npd,), Lh=(npd, npd), Ll=(npd, npd), Lth=(npd, npd), Ltl=(npd, npd), ri=(2, npd),
                  dinv=(2, npd // 64, 64, 64), xh=(ns, 2, npd), xl=(ns, 2, npd))
    out = {name: np.full(shapes[name], sentinel, dtype=np.float64) for name in DDSTAGES_OUT}
    counter = np.full(2, -1, dtype=np.int32)
    rc = load_library().mbfir_test_ddstages(ctx._h, n, U.shape[0], _ptr(H), _ptr(U), _ptr(X), bh.shape[0], _ptr(bh), _ptr(bl), float(pivtol),
                                            DD_FORMS[form], int(nsolve), *[_ptr(out[name]) for name in DDSTAGES_OUT],
                                            counter.ctypes.data_as(_ip))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    out["counter"] = counter
    return out


CAP_SENTINEL = -7.25         # what test_capsolve's output arrays hold on entry (a masked lane's still hold it on return)
CAPSOLVE_OUT = ("M", "Yt", "Zt", "S", "Ms", "rhs_w", "y", "w", "zeta", "dx")


def test_capsolve(H, U, X, a, b, t, k, kp, *, nrhs=None, nlanes=None, mask=None, hsolve_form=-1, sentinel=CAP_SENTINEL, ctx=None):
    """The capacitance form of the extended-precision KKT solve, stage by stage (mbfir_test_capsolve): nl problems
    (H + U' diag(X) U) dx = (a + b) + U' diag(X) t run as one lock-step unit (one problem: as a single design).  H: (nl, n, n); U:
    (nl, kp, n), X: (nl, kp), t: (nl, nrhs, kp), of which lane q's first k[q] rows / entries count; a, b: (nl, nrhs, n); kp: the
    size the launches carry.  hsolve_form: 1 the one-pass M'(M b), 0 the GEMV pair, -1 a solve's own choice.  Returns a dict of the
    padded per-lane intermediates CAPSOLVE_OUT -- M (nl, np, np), Yt, Zt (nl, kp, np), S, Ms (nl, kp, kp), rhs_w, y, dx (nl, nrhs,
    np), w, zeta (nl, nrhs, kp) -- and "flag" (nl replaced-pivot counters), all pre-filled with `sentinel`.  The arguments are
    checked by the library, not here: a bad one raises ValueError with its message."""
    ctx = ctx or get_context()
    H, U, X, a, b, t = [np.ascontiguousarray(v, dtype=np.float64) for v in (H, U, X, a, b, t)]
    k = np.ascontiguousarray(k, dtype=np.int32).ravel()
    nl = int(len(k) if nlanes is None else nlanes)
    n, nv, kp = int(H.shape[-1]), int(a.shape[1] if nrhs is None else nrhs), int(kp)
    npad, kq, nq, vq = -(-n // 64) * 64, max(kp, 1), max(nl, 1), max(nv, 1)
    shapes = {"M": (nq, npad, npad), "Yt": (nq, kq, npad), "Zt": (nq, kq, npad), "S": (nq, kq, kq), "Ms": (nq, kq, kq),
              "rhs_w": (nq, vq, npad), "y": (nq, vq, npad), "w": (nq, vq, kq), "zeta": (nq, vq, kq), "dx": (nq, vq, npad)}
    out = {name: np.full(shapes[name], float(sentinel)) for name in CAPSOLVE_OUT}
    flag = np.full(nq, -1, dtype=np.int32)
    mk = (C.c_int * nq)(*[int(v) for v in mask]) if mask is not None else None
    rc = load_library().mbfir_test_capsolve(ctx._h, n, nl, k.ctypes.data_as(_ip), kp, nv, int(hsolve_form), mk, _ptr(H), _ptr(U), _ptr(X),
                                            _ptr(a), _ptr(b), _ptr(t), *[_ptr(out[name]) for name in CAPSOLVE_OUT],
                                            flag.ctypes.data_as(_ip))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    out["flag"] = flag
    return out


def test_specfact(x, n, ctx=None):
    ctx = ctx or get_context()
    x = _vec(x)
    hre, him = np.zeros(n), np.zeros(n)
    _check(ctx, load_library().mbfir_test_specfact(ctx._h, int(n), _ptr(x), _ptr(hre), _ptr(him)))
    return hre + 1j * him


SPECFACT_BLOCKS = ("in", "work", "h", "hpf", "xl", "xlfp", "a", "lift")


def test_specfact_stages(inp, n=None, *, kind=0, guard=0, fill=0.0, extra=0, ctx=None):
    """Test hook (mbfir_test_specfact_stages): k_specfact (kind 0: inp = nlanes x (2n - 1) reals, one launch with a lane stride) or
    k_fmp (kind 1: inp = an odd number of real or complex taps) through the instantiation that also stores the stages.  Every block
    of the device arena is followed by `guard` doubles of `fill`, `extra` more end each lane.  Returns a dict: lp, lift (per lane),
    st_hpf, st_xl, st_xlfp, st_a, st_h (nlanes x ..., the kernel's own storage order), and to see that nothing outside a block
    changed: raw (nlanes x stride, the arena as the device left it), offsets and sizes (per block name, in doubles)."""
    ctx = ctx or get_context()
    if kind == 0:
        x = np.ascontiguousarray(np.atleast_2d(np.asarray(inp, dtype=np.float64)))
        nlanes = x.shape[0]
        n = (x.shape[1] + 1) // 2 if n is None else int(n)
        if x.ndim != 2 or x.shape[1] != 2 * n - 1:
            raise ValueError("test_specfact_stages: kind 0 takes nlanes x (2n - 1) reals")
        re, im, ntaps = x.ravel(), None, n
    else:
        h = np.asarray(inp).ravel()
        re = np.ascontiguousarray(h.real, dtype=np.float64)
        im = np.ascontiguousarray(h.imag, dtype=np.float64) if np.iscomplexobj(h) else None
        nlanes, n = 1, len(re)
        ntaps = (n + 1) // 2
    lay = np.zeros(18, dtype=np.int64)
    call = lambda raw: load_library().mbfir_test_specfact_stages(                    # noqa: E731
        ctx._h, int(kind), int(n), int(nlanes), _ptr(re), _ptr(im) if im is not None else None, int(guard), float(fill), int(extra),
        lay.ctypes.data_as(_lp), raw)
    rc = call(None)
    if rc == 0:
        raw = np.zeros(nlanes * int(lay[1]), dtype=np.float64)
        rc = call(_ptr(raw))
    if rc == E_ARG:
        raise ValueError(ctx.last_error())
    _check(ctx, rc)
    lp = int(lay[0])
    raw = raw.reshape(nlanes, int(lay[1]))
    off = dict(zip(SPECFACT_BLOCKS, (int(v) for v in lay[2:10])))
    size = dict(zip(SPECFACT_BLOCKS, (int(v) for v in lay[10:18])))
    cplx = lambda k, m: raw[:, off[k]:off[k] + 2 * m:2] + 1j * raw[:, off[k] + 1:off[k] + 2 * m:2]   # noqa: E731
    return dict(lp=lp, lift=raw[:, off["lift"]].copy(), st_hpf=cplx("hpf", lp), st_xl=raw[:, off["xl"]:off["xl"] + lp].copy(),
                st_xlfp=cplx("xlfp", lp), st_a=cplx("a", lp), st_h=cplx("h", ntaps), raw=raw, offsets=off, sizes=size)


def time_kernels(n=1024, m=16394, nt=1023, reps=20, ctx=None):
    """ms per Cholesky+inverse phase (n x n) and per k_gram launch (m x nt) -- tuning aid."""
    ctx = ctx or get_context()
    a, b = C.c_double(), C.c_double()
    _check(ctx, load_library().mbfir_test_time_kernels(ctx._h, n, m, nt, reps, C.byref(a), C.byref(b)))
    return a.value, b.value


def mfma_peak(ctx=None):
    """Measured fp64 MFMA and VALU rates in TFLOP/s (roofline denominators)."""
    ctx = ctx or get_context()
    a, b = C.c_double(), C.c_double()
    _check(ctx, load_library().mbfir_test_mfma_peak(ctx._h, C.byref(a), C.byref(b)))
    return a.value, b.value


def test_fold(w, fold=True):
    """Host-side grid analysis of the lattice kernels (runs without a GPU): dict(ok, nfold, pairs, runs, longest, bad)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = (C.c_long * 6)()
    rc = load_library().mbfir_test_fold(_ptr(w), len(w), 1 if fold else 0, out)
    if rc != 0:
        raise RuntimeError("mbfir_test_fold failed (%d)" % rc)
    return dict(zip(("ok", "nfold", "pairs", "runs", "longest", "bad"), [int(v) for v in out]))
