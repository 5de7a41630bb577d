"""ctypes binding of libcistgcn_hip.so (the C ABI declared in include/cistgcn_hip.h).

There is exactly one backend.  If the library is missing the loader raises; nothing in this
package computes on the CPU or through stock PyTorch operators instead.

The Structure classes, `LIMITS` and `_SIGNATURES` below are written by hand after the header the kernels are compiled
against.  tests/test_boundary.py holds them to it: every size, field offset, field size and macro value against a C++
program that includes the header, every argument list against its prototype.
"""
import ctypes
import os
from ctypes import POINTER, c_double, c_float, c_int, c_int32, c_longlong, c_uint, c_ulonglong, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcistgcn_hip.so")

_handle = None
# Limits a caller of the ABI has to honour, by their macro names in include/cistgcn_hip.h.
LIMITS = {
    "CG_STAT_REPLICAS": 16,      # replicas of a BatchNorm channel-sum buffer
    "CG_ALPHA_SLOTS": 64,        # f64 words the partial sums of a shared PReLU slope's gradient are spread over
    "CG_MAX_BATCH": 16,          # problems per cg_contract_many launch
    "CG_ROW_MAX_BATCH": 6,       # problems per launch of the row kernels
    "CG_SUM_MAX": 8,             # addends per cg_sum_many launch
    "CG_COPY_MAX": 4,            # copies per cg_copy_many launch
    "CG_BIN_MAXG": 8,            # consumer gradients per cg_block_input_bwd
    "CG_MID_MAXN": 6,            # items per cg_block_mid_* launch
    "CG_PWM_MAXN": 4,            # cg_pointwise_maps_*: maps per launch,
    "CG_PWM_MAXROWS": 128,       # their output channels (each rounded up to 16) together,
    "CG_PWM_MAXCIN": 128,        # input channels,
    "CG_PWM_MAXM": 64,           # output channels of one map
    "CG_GATE_MAXC": 64,          # cg_gate_head_*: channels,
    "CG_GATE_MAXS": 192,         # block statistics per sample
    "CG_CTX_MAXC": 64,           # channels of cg_context_heads_*
    "CG_EM_METRICS": 9,          # outputs of cg_eval_metrics
    "CG_AM_OUT": 33,             # outputs of cg_attack_metrics,
    "CG_AM_BINS": 64,            # bins of its histograms
    "CG_PERTURB_MAX_STEPS": 16,  # steps per cg_perturb_sequences launch, and the step kinds of its table:
    "CG_PERTURB_ROTATION": 0, "CG_PERTURB_SCALE": 1, "CG_PERTURB_NOISE": 2, "CG_PERTURB_TRANSLATION": 3, "CG_PERTURB_FLIP": 4,
    "CG_PERTURB_INVERT": 5,
    # kinds of cg_motion_loss_*, the threads of its workgroups (64 per frame in flight) and the cap of its grid = f64 words of its scratch
    "CG_LOSS_WEIGHTED_MPJPE": 0, "CG_LOSS_MPJPE_SOFT": 1, "CG_LOSS_WEIGHTED_MPJPE_SOFT": 2, "CG_LOSS_RMPJPE": 3,
    "CG_LOSS_THREADS": 256, "CG_LOSS_MAX_BLOCKS": 512,
    # cg_forward_kinematics: joints of a tree (and of `select`), the cap of its grid, the threads of a workgroup (64 per one or two frames
    # in flight) and its two conventions
    "CG_FK_MAX_JOINTS": 64, "CG_FK_MAX_BLOCKS": 1024, "CG_FK_THREADS": 256, "CG_FK_EXPMAP_CHAIN": 0, "CG_FK_SMPL": 1,
    # cg_draw_augmentation: the first salt of its generator (dropout site ids stay below it), its two table layouts, the threads of a
    # workgroup and the cap of its grid
    "CG_DRAW_SALT": 0x800000, "CG_DRAW_TABLE24": 0, "CG_DRAW_STEPS4": 1, "CG_DRAW_THREADS": 256, "CG_DRAW_MAX_BLOCKS": 4096,
}
STAT_REPLICAS = LIMITS["CG_STAT_REPLICAS"]
ALPHA_SLOTS = LIMITS["CG_ALPHA_SLOTS"]
# Host pointers are refused unless a test harness has injected an emulated build of the very same
# kernel sources (tests/hipemu).  The product never sets this.
_host_pointers_ok = False


class View4(ctypes.Structure):
    _fields_ = [("n", c_longlong * 4), ("s", c_longlong * 4)]


class NormAct(ctypes.Structure):
    _fields_ = [
        ("x", c_void_p), ("xv", View4),
        ("y", c_void_p), ("yv", View4),
        ("pre", c_void_p),
        ("add", c_void_p), ("av", View4),
        ("add_post", c_int),
        ("bn_mode", c_int),
        ("stats", c_void_p),
        ("gamma", c_void_p), ("beta", c_void_p),
        ("running_mean", c_void_p), ("running_var", c_void_p), ("num_batches_tracked", c_void_p),
        ("momentum", c_float), ("eps", c_float),
        ("save_mean", c_void_p), ("save_rstd", c_void_p),
        ("drop_p", c_float), ("seed", c_void_p), ("salt", c_uint),
        ("alpha", c_void_p), ("alpha_n", c_int),
        ("dy", c_void_p), ("dyv", View4),
        ("dx", c_void_p), ("dxv", View4),
        ("dadd", c_void_p), ("dav", View4),
        ("dpre", c_void_p),
        ("red", c_void_p),
        ("dgamma", c_void_p), ("dbeta", c_void_p), ("dalpha", c_void_p),
        ("ystats", c_void_p),
    ]


class ContractDesc(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("X", c_void_p), ("Y", c_void_p), ("bias", c_void_p), ("stats", c_void_p), ("tab", c_void_p),
                ("G", c_int), ("M", c_int), ("N", c_int), ("K", c_int), ("splitk", c_int), ("kchunk", c_int),
                ("a_kfast", c_int), ("x_kfast", c_int), ("accumulate", c_int), ("x_vec", c_int), ("stat_ch", c_int), ("mode", c_int), ("block0", c_longlong),
                ("ws", c_void_p), ("chain", c_int), ("pad2", c_int)]


class StatsArgs(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("xv", View4), ("pre", c_void_p), ("stats", c_void_p)]


class SumItem(ctypes.Structure):
    _fields_ = [("a", c_void_p), ("av", View4)]


class Rank1(ctypes.Structure):
    _fields_ = [("s", c_void_p), ("q", c_void_p), ("o", c_void_p), ("dout", c_void_p), ("ds", c_void_p), ("dq", c_void_p),
                ("domain", c_int), ("pad", c_int)]


class CopyItem(ctypes.Structure):
    _fields_ = [("y", c_void_p), ("yv", View4), ("a", c_void_p), ("av", View4)]


class TailBN(ctypes.Structure):
    _fields_ = [("stats", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("num_batches_tracked", c_void_p), ("momentum", c_float), ("eps", c_float), ("save", c_void_p)]


class DstdTail(ctypes.Structure):
    _fields_ = [("B", c_int), ("C", c_int), ("T", c_int), ("V", c_int), ("train", c_int), ("pad0", c_int),
                ("y", c_void_p * 2), ("r", c_void_p * 2), ("w", c_void_p * 2),
                ("bn_t", TailBN * 2), ("alpha_d", c_void_p * 2),
                ("bn_p", TailBN * 2), ("alpha_p", c_void_p * 2),
                ("Wc", c_void_p), ("bn_c", TailBN), ("alpha_c", c_void_p),
                ("gate", c_void_p), ("bres", c_void_p),
                ("drop_p", c_float), ("salt", c_uint * 2), ("pad1", c_int), ("seed", c_void_p),
                ("h0", c_void_p), ("pooled", c_void_p), ("out", c_void_p), ("ostats", c_void_p),
                ("tap_x", c_void_p * 2), ("tap_a", c_void_p * 2), ("tap_h", c_void_p),
                ("dout", c_void_p), ("dpooled", c_void_p), ("dgate", c_void_p), ("red_c", c_void_p),
                ("gp", c_void_p * 2), ("red_p", c_void_p * 2), ("dWc_ws", c_void_p), ("dWc", c_void_p),
                ("dr", c_void_p * 2), ("dw", c_void_p * 2), ("red_t", c_void_p * 2), ("dy", c_void_p * 2),
                ("dgamma_t", c_void_p * 2), ("dbeta_t", c_void_p * 2), ("dalpha_d", c_void_p * 2),
                ("dgamma_p", c_void_p * 2), ("dbeta_p", c_void_p * 2), ("dalpha_p", c_void_p * 2),
                ("dgamma_c", c_void_p), ("dbeta_c", c_void_p), ("dalpha_c", c_void_p),
                ("rows_c", c_void_p), ("fmom", c_void_p * 2), ("red_q", c_void_p * 2), ("rs_shared", c_int), ("pad2", c_int)]


class AdjTail(ctypes.Structure):
    _fields_ = [("B", c_int), ("Kc", c_int), ("J", c_int), ("domain", c_int), ("train", c_int), ("pad0", c_int),
                ("s", c_void_p), ("q", c_void_p), ("W0", c_void_p), ("bn", TailBN), ("alpha", c_void_p), ("W4", c_void_p),
                ("drop_p", c_float), ("salt", c_uint), ("seed", c_void_p),
                ("e", c_void_p), ("adj", c_void_p), ("tap", c_void_p),
                ("dadj", c_void_p), ("g", c_void_p), ("red", c_void_p), ("ds", c_void_p), ("dq", c_void_p), ("part", c_void_p),
                ("dW0_ws", c_void_p), ("dW4_ws", c_void_p),
                ("dW0", c_void_p), ("dW4", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("dalpha", c_void_p)]


class PwMaps(ctypes.Structure):
    _fields_ = [("B", c_int), ("Cin", c_int), ("P", c_int), ("n", c_int), ("x", c_void_p),
                ("W", c_void_p * 4), ("M", c_int * 4), ("y", c_void_p * 4), ("stats", c_void_p * 4),
                ("dy", c_void_p * 4), ("dx", c_void_p), ("dW", c_void_p * 4), ("dW_ws", c_void_p),
                ("bias", c_void_p * 4), ("db", c_void_p * 4),
                ("yraw", c_void_p * 4), ("bn_save", c_void_p * 4), ("bn_gamma", c_void_p * 4), ("bn_beta", c_void_p * 4),
                ("bn_red", c_void_p * 4), ("prelu", c_void_p * 4), ("bn_train", c_int), ("pad", c_int)]


class FpnConv(ctypes.Structure):
    _fields_ = [("B", c_int), ("C", c_int), ("O", c_int), ("H", c_int), ("W", c_int), ("n", c_int), ("dil", c_int * 3), ("pad", c_int),
                ("x", c_void_p), ("xs", c_longlong * 3), ("w", c_void_p * 3), ("bias", c_void_p * 3), ("y", c_void_p * 3),
                ("dy", c_void_p * 3), ("dx", c_void_p), ("dw", c_void_p * 3), ("db", c_void_p * 3), ("ws", c_void_p)]


class RowsConv(ctypes.Structure):
    _fields_ = [("B", c_int), ("C", c_int), ("T", c_int), ("V", c_int), ("O", c_int), ("pad", c_int),
                ("x", c_void_p), ("W", c_void_p), ("y", c_void_p), ("stats", c_void_p),
                ("dy", c_void_p), ("dx", c_void_p), ("dW", c_void_p), ("ws", c_void_p),
                ("in_on", c_int), ("in_train", c_int), ("in_bn", TailBN), ("in_alpha", c_void_p), ("in_tap", c_void_p),
                ("sums", c_void_p), ("red", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("dalpha", c_void_p)]


class BlockInput(ctypes.Structure):
    _fields_ = [("B", c_int), ("C", c_int), ("T", c_int), ("V", c_int), ("train", c_int), ("ng", c_int),
                ("x", c_void_p), ("bn", TailBN), ("xn", c_void_p), ("rm", c_void_p), ("rq", c_void_p), ("out", c_void_p),
                ("g", c_void_p * 8), ("dout", c_void_p * 2), ("dout_ld", c_longlong * 2), ("pq", c_void_p), ("gsum", c_void_p), ("red", c_void_p),
                ("dx", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p)]


class GatePath(ctypes.Structure):
    _fields_ = [("z", c_void_p), ("stats", c_void_p), ("stats_ld", c_longlong),
                ("bn2", TailBN), ("alpha2", c_void_p), ("Wl", c_void_p), ("bn3", TailBN), ("alpha3", c_void_p), ("W2", c_void_p),
                ("salt2", c_uint), ("salt3", c_uint), ("y", c_void_p), ("w", c_void_p), ("tap2", c_void_p), ("tap3", c_void_p),
                ("dw", c_void_p), ("dz", c_void_p), ("dstats", c_void_p), ("dWl", c_void_p), ("dW2", c_void_p),
                ("dgamma2", c_void_p), ("dbeta2", c_void_p), ("dalpha2", c_void_p), ("dgamma3", c_void_p), ("dbeta3", c_void_p), ("dalpha3", c_void_p),
                ("scratch", c_void_p), ("red", c_void_p)]


class GateHead(ctypes.Structure):
    _fields_ = [("B", c_int), ("C", c_int), ("S", c_int), ("train", c_int), ("n", c_int), ("pad", c_int),
                ("drop_p", c_float), ("pad2", c_int), ("seed", c_void_p), ("p", GatePath * 2)]


class MidItem(ctypes.Structure):
    _fields_ = [("kind", c_int), ("C", c_int), ("L", c_int), ("O", c_int), ("sb_", c_int), ("ns_", c_int),
                ("x", c_void_p), ("x_ld", c_longlong), ("bn", TailBN), ("stats_ld", c_longlong), ("alpha", c_void_p), ("W", c_void_p),
                ("salt", c_uint), ("pad", c_int), ("y", c_void_p), ("tap", c_void_p),
                ("dy", c_void_p), ("dx", c_void_p), ("dW", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("dalpha", c_void_p),
                ("g", c_void_p), ("part", c_void_p), ("wpart", c_void_p)]


class BlockMid(ctypes.Structure):
    _fields_ = [("B", c_int), ("train", c_int), ("n", c_int), ("pad", c_int),
                ("drop_p", c_float), ("pad2", c_int), ("seed", c_void_p), ("it", MidItem * 6)]


class CtxHeads(ctypes.Structure):
    _fields_ = [("B", c_int), ("P", c_int), ("C", c_int), ("train", c_int), ("x", c_void_p), ("xstats", c_void_p),
                ("w", c_void_p * 2), ("bn", TailBN * 2), ("alpha", c_void_p * 2),
                ("y", c_void_p * 2), ("arg", c_void_p), ("xsave", c_void_p), ("tap", c_void_p * 2),
                ("dy", c_void_p * 2), ("red", c_void_p), ("dx", c_void_p),
                ("dw", c_void_p * 2), ("dgamma", c_void_p * 2), ("dbeta", c_void_p * 2), ("dalpha", c_void_p * 2)]


class AttackStep(ctypes.Structure):
    _fields_ = [("B", c_int), ("T", c_int), ("V", c_int), ("mode", c_int), ("iterations", c_int), ("patience", c_int),
                ("epsilon", c_float), ("mu", c_float),
                ("x0", c_void_p), ("x", c_void_p), ("grad", c_void_p), ("g", c_void_p), ("mask", c_void_p), ("loss", c_void_p),
                ("best", c_void_p), ("stall", c_void_p), ("active", c_void_p), ("w", c_void_p), ("queries", c_void_p), ("n_active", c_void_p),
                ("steps", c_void_p), ("frozen_at", c_void_p)]


class DeepfoolStep(ctypes.Structure):
    _fields_ = [("B", c_int), ("T", c_int), ("To", c_int), ("V", c_int), ("patience", c_int), ("pad", c_int),
                ("x", c_void_p), ("grad", c_void_p), ("pred", c_void_p), ("mask", c_void_p), ("loss", c_void_p),
                ("best", c_void_p), ("stall", c_void_p), ("active", c_void_p), ("w", c_void_p), ("queries", c_void_p), ("n_active", c_void_p),
                ("steps", c_void_p), ("frozen_at", c_void_p)]


class EvalMetricsArgs(ctypes.Structure):
    _fields_ = [("B", c_int), ("To", c_int), ("J", c_int), ("Nb", c_int), ("frames", c_int), ("pad", c_int),
                ("pred", c_void_p), ("target", c_void_p), ("speeds", c_void_p), ("bones", c_void_p),
                ("out", c_void_p * 9), ("ws", c_void_p)]


class AttackMetricsArgs(ctypes.Structure):
    _fields_ = [("B", c_int), ("T", c_int), ("J", c_int), ("pad", c_int),
                ("adv", c_void_p), ("orig", c_void_p), ("out", c_void_p * 33), ("counts", c_void_p), ("gmax", c_void_p), ("ws", c_void_p)]


class MotionLoss(ctypes.Structure):
    _fields_ = [("kind", c_int), ("B", c_int), ("T", c_int), ("V", c_int), ("speed_factor", c_float), ("pad", c_int),
                ("pred", c_void_p), ("target", c_void_p), ("w_full", c_void_p), ("w_frame", c_void_p), ("speeds", c_void_p),
                ("part", c_void_p), ("loss", c_void_p), ("mean", c_void_p), ("gloss", c_void_p), ("dpred", c_void_p)]


class ForwardKinematics(ctypes.Structure):
    _fields_ = [("convention", c_int), ("J", c_int), ("J_pose", c_int), ("J_out", c_int), ("N", c_longlong), ("scale", c_float), ("pad", c_int),
                ("angles", c_void_p), ("parent", c_void_p), ("rest", c_void_p), ("select", c_void_p), ("out", c_void_p)]


class GatherWindows(ctypes.Structure):
    _fields_ = [("B", c_int), ("L", c_int), ("J_src", c_int), ("J", c_int), ("W", c_int), ("up_hi", c_int), ("up_lo", c_int), ("pad", c_int),
                ("F", c_longlong), ("mean", c_float), ("std", c_float),
                ("frames", c_void_p), ("starts", c_void_p), ("items", c_void_p), ("select", c_void_p), ("raw", c_void_p)]


class DrawStep(ctypes.Structure):
    _fields_ = [("kind", c_int), ("prob_threshold", c_float), ("lo", c_float * 3), ("hi", c_float * 3)]


# A class mirrors the header's struct "Cg" + its own name, except these two.
C_STRUCT_NAMES = {"EvalMetricsArgs": "CgEvalMetrics", "AttackMetricsArgs": "CgAttackMetrics"}


P = c_void_p
LL = c_longlong
_SIGNATURES = {
    "cg_contract": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, LL, P],
    "cg_contract_many": [POINTER(ContractDesc), c_int, P],
    "cg_contract_kred_ws_floats": [c_int, c_int, c_int],
    "cg_chan_stats": [P, POINTER(View4), P, P, P],
    "cg_chan_stats_many": [POINTER(StatsArgs), c_int, P],
    "cg_norm_act_fwd_many": [POINTER(NormAct), c_int, P],
    "cg_norm_act_bwd_many": [POINTER(NormAct), POINTER(c_int), c_int, P],
    "cg_norm_act_bwd_reduce_many": [POINTER(NormAct), c_int, P],
    "cg_copy_many": [POINTER(CopyItem), c_int, P],
    "cg_chan_sum": [P, POINTER(View4), P, P],
    "cg_norm_act_fwd": [POINTER(NormAct), P],
    "cg_norm_act_bwd": [POINTER(NormAct), c_int, P],
    "cg_reduce_bc": [P, POINTER(View4), c_int, P, P, P],
    "cg_reduce_bc_bwd": [P, P, c_int, P, POINTER(View4), P],
    "cg_sum_many": [P, POINTER(View4), POINTER(SumItem), c_int, P],
    "cg_rank1_adj_fwd": [POINTER(Rank1), c_int, c_int, c_int, c_int, P],
    "cg_rank1_adj_bwd": [POINTER(Rank1), c_int, c_int, c_int, c_int, P],
    "cg_gather_joints": [P, P, P, LL, c_int, c_int, P],
    "cg_eval_scatter_mpjpe": [P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "cg_add3": [P, POINTER(View4), P, POINTER(View4), P, POINTER(View4), P, POINTER(View4), P],
    "cg_zero": [P, LL, P],
    "cg_feature_lift_fwd": [P, P, LL, LL, LL, P],
    "cg_feature_lift_bwd": [P, P, P, LL, LL, LL, P],
    "cg_dstd_stats_fwd": [P, P, c_int, c_int, c_int, c_int, P],
    "cg_dstd_stats_bwd": [P, P, P, c_int, c_int, c_int, c_int, P],
    "cg_se_gate_fwd": [P, P, P, P, c_int, c_int, c_int, P],
    "cg_se_gate_bwd": [P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "cg_cumsum": [P, POINTER(View4), P, POINTER(View4), c_int, P],
    "cg_mpjpe_fwd": [P, P, P, LL, P],
    "cg_mpjpe_bwd": [P, P, P, P, LL, P],
    "cg_seed_bump": [P, P],
    "cg_stgcn_domain_fwd": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "cg_stgcn_domain_bwd": [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "cg_stgcn_domain_bwd_ws_floats": [c_int, c_int],
    "cg_stgcn_domain_planes_min_workgroups": [c_longlong],
    "cg_multi_copy": [P, P, P, P, P, c_int, P, c_int, c_float, P],
    "cg_scale": [P, LL, c_float, P],
    "cg_dstd_tail_fwd": [POINTER(DstdTail), c_int, P],
    "cg_dstd_tail_bwd": [POINTER(DstdTail), c_int, P],
    "cg_dstd_tail_ws_floats": [c_int],
    "cg_collapse_rows_fwd": [POINTER(RowsConv), P],
    "cg_collapse_rows_bwd": [POINTER(RowsConv), P],
    "cg_collapse_rows_ws_floats": [c_int, c_int, c_int],
    "cg_collapse_cols_fwd": [POINTER(RowsConv), P],
    "cg_collapse_cols_bwd": [POINTER(RowsConv), P],
    "cg_collapse_cols_supported": [c_int, c_int, c_int, c_int],
    "cg_collapse_cols_ws_floats": [c_int, c_int, c_int],
    "cg_collapse_sums_ws_floats": [c_int, c_int],
    "cg_fpn_conv_fwd": [POINTER(FpnConv), P],
    "cg_fpn_conv_bwd": [POINTER(FpnConv), P],
    "cg_fpn_conv_supported": [c_int, c_int, c_int, c_int, c_int],
    "cg_fpn_conv_ws_floats": [c_int, c_int, c_int, c_int],
    "cg_pointwise_maps_fwd": [POINTER(PwMaps), P],
    "cg_pointwise_maps_bwd": [POINTER(PwMaps), P],
    "cg_pointwise_maps_ws_floats": [c_int],
    "cg_block_input_fwd": [POINTER(BlockInput), P],
    "cg_block_input_bwd": [POINTER(BlockInput), P],
    "cg_block_input_supported": [c_int, c_int, c_int, c_int],
    "cg_gate_head_fwd": [POINTER(GateHead), P],
    "cg_gate_head_bwd": [POINTER(GateHead), P],
    "cg_gate_head_supported": [c_int, c_int, c_int],
    "cg_gate_head_scratch_floats": [c_int, c_int, c_int],
    "cg_block_mid_fwd": [POINTER(BlockMid), P],
    "cg_block_mid_bwd": [POINTER(BlockMid), P],
    "cg_block_mid_supported": [c_int, c_int, c_int, c_int, c_int],
    "cg_block_mid_geometry": [c_int, c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_context_heads_fwd": [POINTER(CtxHeads), P],
    "cg_context_heads_bwd": [POINTER(CtxHeads), P],
    "cg_context_heads_red_doubles": [c_int],
    "cg_map2adj_tail_fwd": [POINTER(AdjTail), c_int, c_int, P],
    "cg_map2adj_tail_bwd": [POINTER(AdjTail), c_int, c_int, P],
    "cg_map2adj_tail_ws_floats": [c_int],
    "cg_map2adj_tail_part_floats": [c_int, c_int, c_int],
    "cg_map2adj_tail_red_doubles": [c_int],
    "cg_augment_sequences": [P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "cg_perturb_sequences": [P, POINTER(c_int), P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "cg_map2adj_tail_geometry": [c_int, c_int, c_int, POINTER(c_int)],
    "cg_dstd_tail_geometry": [c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_pointwise_maps_geometry": [c_int, c_int, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int)],
    "cg_collapse_geometry": [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_fpn_conv_geometry": [c_int, c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_stgcn_domain_geometry": [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_block_input_geometry": [c_int, c_int, c_int, c_int, POINTER(c_int)],
    "cg_norm_act_rows_per_block": [POINTER(View4)],
    "cg_glue_geometry": [c_int, c_int, c_int, POINTER(c_int)],
    "cg_mpjpe_sample_fwd": [P, P, P, c_int, c_int, P],
    "cg_mpjpe_sample_bwd": [P, P, P, P, c_int, c_int, P],
    "cg_attack_step": [POINTER(AttackStep), P],
    "cg_attack_step_max_floats": [],
    "cg_deepfool_step": [POINTER(DeepfoolStep), P],
    "cg_eval_metrics": [POINTER(EvalMetricsArgs), P],
    "cg_eval_metrics_ws_doubles": [c_int, c_int, c_int],
    "cg_attack_metrics": [POINTER(AttackMetricsArgs), P],
    "cg_attack_metrics_ws_doubles": [c_int, c_int, c_int],
    "cg_motion_loss_fwd": [POINTER(MotionLoss), P],
    "cg_motion_loss_bwd": [POINTER(MotionLoss), P],
    "cg_forward_kinematics": [POINTER(ForwardKinematics), P],
    "cg_gather_windows": [POINTER(GatherWindows), P],
    "cg_gather_windows_at": [POINTER(GatherWindows), P, P, P],
    "cg_cursor_advance": [P, c_int, P],
    "cg_draw_augmentation": [POINTER(DrawStep), c_int, P, c_int, c_int, c_int, c_int, P, P, P],
    "cg_adam_flat": [P, P, P, P, LL, c_float, c_float, c_float, c_float, c_float, c_float, c_float, LL, P],
}
EXPORTS = tuple(sorted(_SIGNATURES))


def declare(handle):
    """Attach argument/return types for every entry point of include/cistgcn_hip.h."""
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(handle, name)     # AttributeError if the library does not export it
        fn.argtypes = argtypes
        fn.restype = c_longlong if name.endswith(("_floats", "_doubles", "_workgroups")) else c_int
    return handle


def lib():
    """The loaded kernel library; raises RuntimeError if it has not been built."""
    global _handle
    if _handle is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "cistgcn_amd: %s is missing. Build it with `python -m cistgcn_amd.build` "
                "(hipcc --offload-arch=gfx950); there is no fallback implementation." % LIB_PATH)
        _handle = declare(ctypes.CDLL(LIB_PATH))
    return _handle


_STATUS = {-1: "bad argument (null pointer / option without its buffer)", -2: "unsupported shape"}


def check(status, name):
    if status != 0:
        what = _STATUS.get(status, "hipError_t %d" % status)
        raise RuntimeError("cistgcn_hip: %s failed: %s" % (name, what))


def call(name, *args):
    check(getattr(lib(), name)(*args), name)
