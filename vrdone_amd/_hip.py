"""ctypes binding of libvrdone_hip.so (C ABI declared in include/vrdone_hip.h).

There is no CPU fallback: importing this module without the built library, or calling an
op on a non-HIP tensor, raises.  Build with ``make -C vrdone_amd/csrc`` (or
``python -c "import __graft_entry__ as g; g.build()"``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VRDONE_HIP_LIB: another build of the same library (kernel experiments, A/B runs in one box session)
LIB_PATH = os.environ.get("VRDONE_HIP_LIB") or os.path.join(_HERE, "csrc", "libvrdone_hip.so")

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
PAIR_NONE, PAIR_BF16, PAIR_F16 = 0, 1, 2          # enum vrd_pair_format
F16_ACT_EXP = 4                                   # VRD_F16_ACT_EXP
ABSMAX_SCALE_FLOATS = 516                         # VRD_ABSMAX_SCALE_FLOATS: vrd_absmax_scale's buffer (factors, ticket, partial maxima)
ADAMW_GROUP_FLOATS = 8                            # VRD_ADAMW_GROUP_FLOATS: one row of vrd_adamw_step's hyper-parameter table
(K_GEMM, K_LAYERNORM, K_DWCONV_LN, K_LOCAL_ATTN, K_ATTN_SMALL, K_ATTN_FLASH, K_POOL, K_MASK_HEAD,
 K_TRANSPOSE, K_POSTPROC, K_GEMM_X3, K_GEMM_X3_DMA, K_GEMM_X3_BIG, K_BACKWARD, K_COUNT) = range(15)   # enum vrd_kernel_id
KERNEL_NAMES = ["gemm_f32_mfma", "layernorm", "dwconv_ln", "local_attn", "attn_small", "attn_flash",
                "maxpool_mask", "mask_head", "transpose", "postprocess", "gemm_x3_mfma", "gemm_x3_dma",
                "gemm_x3_big", "backward"]
assert len(KERNEL_NAMES) == K_COUNT

c_f32p = C.c_void_p      # device pointers travel as plain integers
c_u8p = C.c_void_p
c_i32p = C.c_void_p


class CriterionArgs(C.Structure):                     # vrd_criterion_args
    _fields_ = [("logits", C.c_void_p * 4), ("masks", C.c_void_p * 4),
                ("n_layers", C.c_int32), ("B", C.c_int32), ("Q", C.c_int32), ("K1", C.c_int32), ("T", C.c_int32), ("G", C.c_int32),
                ("out_valid", C.c_void_p), ("tgt_ids", C.c_void_p), ("tgt_masks", C.c_void_p), ("owner", C.c_void_p),
                ("segs", C.c_void_p), ("scale_range", C.c_float), ("alpha", C.c_float), ("gamma", C.c_float),
                ("w_class", C.c_float), ("w_mask", C.c_float), ("w_dice", C.c_float)]


class CriterionGrads(C.Structure):                    # vrd_criterion_grads
    _fields_ = [("logits", C.c_void_p * 4), ("masks", C.c_void_p * 4)]


class GemmArgs(C.Structure):
    _fields_ = [("A", c_f32p), ("lda", C.c_int64), ("W", c_f32p), ("bias", c_f32p),
                ("C", c_f32p), ("ldc", C.c_int64),
                ("M", C.c_int64), ("N", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32), ("T", C.c_int32),
                ("act", C.c_int32), ("row_mask", c_u8p), ("scale", c_f32p),
                ("res", c_f32p), ("ldres", C.c_int64), ("res_masked", C.c_int32),
                ("res2", c_f32p), ("ldres2", C.c_int64), ("W_split", C.c_void_p),
                ("a_pair_width", C.c_int32), ("c_pair", C.c_int32),
                ("row_blocks", C.c_void_p), ("row_blocks_active", C.c_void_p), ("row_block_seg_len", C.c_int32),
                ("split_fmt", C.c_int32), ("w_scale", c_f32p), ("a_scale", c_f32p), ("products", C.c_int32)]


MAX_SEGS = 32                                     # VRD_MAX_SEGS


class RowSegs(C.Structure):
    """vrd_row_segs: a ragged row space as groups of sequences (n[i] sequences of T[i] frames from row row[i] on)"""
    _fields_ = [("count", C.c_int32), ("n", C.c_int32 * MAX_SEGS), ("T", C.c_int32 * MAX_SEGS), ("row", C.c_int64 * MAX_SEGS)]

    _made = {}

    @classmethod
    def of(cls, segs):
        """segs: [(first row, sequences, frames)]; the structs are read-only and kept (a network pass asks for the same few
        tables ~25 times)"""
        key = tuple(segs)
        s = cls._made.get(key)
        if s is None:
            assert 1 <= len(segs) <= MAX_SEGS
            if len(cls._made) > 4096:
                cls._made.clear()
            s = cls._made[key] = cls()
            s.count = len(segs)
            for i, (row, n, T) in enumerate(segs):
                s.row[i], s.n[i], s.T[i] = row, n, T
        return s


class DwconvLnArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("ldx", C.c_int64), ("x_up", c_f32p), ("ldx_up", C.c_int64),
                ("B", C.c_int32), ("Tin", C.c_int32), ("C", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("group_in", C.c_int32),
                ("mask_out", c_u8p), ("n_out", C.c_int32),
                ("w", c_f32p * 3), ("bias", c_f32p * 3), ("gamma", c_f32p * 3), ("beta", c_f32p * 3),
                ("relu", C.c_int32 * 3), ("y", c_f32p * 3), ("ldy", C.c_int64 * 3), ("out_pair", C.c_int32 * 3),
                ("pre_gamma", c_f32p), ("pre_beta", c_f32p), ("packed", c_f32p * 3), ("segs", C.POINTER(RowSegs))]


DWCONV_MULTI_SETS = 5                             # VRD_DWCONV_MULTI_SETS


class DwconvLnMultiArgs(C.Structure):                 # vrd_dwconv_ln_multi_args
    _fields_ = [("x", c_f32p), ("ldx", C.c_int64), ("B", C.c_int32), ("Tin", C.c_int32), ("C", C.c_int32),
                ("mask_out", c_u8p), ("n_out", C.c_int32),
                ("packed", c_f32p * DWCONV_MULTI_SETS), ("has_ln", C.c_int32 * DWCONV_MULTI_SETS),
                ("relu", C.c_int32 * DWCONV_MULTI_SETS), ("pre_ln", C.c_int32 * DWCONV_MULTI_SETS),
                ("y", c_f32p * DWCONV_MULTI_SETS), ("ldy", C.c_int64 * DWCONV_MULTI_SETS),
                ("out_pair", C.c_int32 * DWCONV_MULTI_SETS),
                ("pre_gamma", c_f32p), ("pre_beta", c_f32p), ("segs", C.POINTER(RowSegs))]


class ConvLnArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("ldx", C.c_int64), ("rows", C.c_int64),
                ("Cin", C.c_int32), ("taps", C.c_int32), ("T", C.c_int32), ("N", C.c_int32),
                ("w", c_f32p), ("bias", c_f32p), ("row_mask", c_u8p), ("gamma", c_f32p), ("beta", c_f32p),
                ("relu", C.c_int32), ("y", c_f32p), ("ldy", C.c_int64), ("out_pair", C.c_int32)]


class PackArgs(C.Structure):
    _fields_ = [("src", C.c_void_p), ("lens", C.c_void_p),
                ("P", C.c_int32), ("C_in", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("Cc", C.c_int32),
                ("S", C.c_int32), ("E", C.c_int32),
                ("vis", c_f32p), ("clip", c_f32p), ("so_box", c_f32p), ("ent", c_f32p), ("pair_wide", C.c_int32)]


class DwconvBwdArgs(C.Structure):
    _fields_ = [("dD", c_f32p * 3), ("lddd", C.c_int64 * 3), ("w", c_f32p * 3),
                ("n_out", C.c_int32), ("B", C.c_int32), ("Tin", C.c_int32), ("C", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("group_in", C.c_int32),
                ("mask_out", c_u8p), ("dx", c_f32p), ("lddx", C.c_int64), ("dx_up", c_f32p), ("lddx_up", C.c_int64)]


class BmmArgs(C.Structure):
    _fields_ = [("A", c_f32p), ("a_z0", C.c_int64), ("a_z1", C.c_int64), ("a_row", C.c_int64), ("a_col", C.c_int64),
                ("B", c_f32p), ("b_z0", C.c_int64), ("b_z1", C.c_int64), ("b_row", C.c_int64), ("b_col", C.c_int64),
                ("C", c_f32p), ("c_z0", C.c_int64), ("c_z1", C.c_int64), ("c_row", C.c_int64), ("c_col", C.c_int64),
                ("Z0", C.c_int32), ("Z1", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("alpha", C.c_float), ("accumulate", C.c_int32)]


class SplitJob(C.Structure):
    _fields_ = [("src", c_f32p), ("out", C.c_void_p), ("R", C.c_int32), ("Q", C.c_int32), ("taps", C.c_int32), ("fmt", C.c_int32),
                ("sr", C.c_int64), ("st", C.c_int64), ("sq", C.c_int64), ("scale", c_f32p)]


class GatherArgs(C.Structure):
    _fields_ = [("vis", c_f32p), ("clip", c_f32p), ("boxes", c_f32p), ("s_row", C.c_void_p), ("o_row", C.c_void_p),
                ("lens", C.c_void_p), ("P", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("Cc", C.c_int32),
                ("stride", C.c_int32), ("w", C.c_float), ("h", C.c_float),
                ("out_vis", c_f32p), ("out_clip", c_f32p), ("out_so_box", c_f32p), ("out_ent", c_f32p),
                ("pair_wide", C.c_int32), ("seq_wh", c_f32p)]


class GatherTrainArgs(C.Structure):                   # vrd_gather_train_args
    _fields_ = [("vis", c_f32p), ("clip", c_f32p), ("boxes", c_f32p), ("s_row", C.c_void_p), ("o_row", C.c_void_p),
                ("lens", C.c_void_p), ("lead", C.c_void_p), ("seq_wh", c_f32p), ("seg_lo", C.c_void_p), ("seg_hi", C.c_void_p),
                ("P", C.c_int32), ("G", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("Cc", C.c_int32), ("stride", C.c_int32),
                ("out_vis", c_f32p), ("out_clip", c_f32p), ("out_so_box", c_f32p), ("out_ent", c_f32p), ("out_mask", c_u8p),
                ("out_targets", c_f32p), ("pair_wide", C.c_int32)]


class SelectArgs(C.Structure):                        # vrd_select_args
    _fields_ = [("cand", c_f32p), ("s_score", c_f32p), ("o_score", c_f32p), ("so_offset", c_i32p), ("so_start", c_i32p),
                ("so_end", c_i32p), ("video_pairs", c_i32p),
                ("n_videos", C.c_int32), ("max_video_pairs", C.c_int32), ("Q", C.c_int32), ("k", C.c_int32),
                ("feat_stride", C.c_int32), ("pred_min_frames", C.c_int32), ("n_max_pair", C.c_int32),
                ("out_count", c_i32p), ("out_index", c_i32p), ("out_score", c_f32p)]


class ViouArgs(C.Structure):                          # vrd_viou_args
    _fields_ = [("pred_boxes", c_f32p), ("pred_rows", C.c_int64), ("gt_boxes", c_f32p), ("gt_rows", C.c_int64),
                ("pred", C.c_void_p), ("gt", C.c_void_p), ("cand", c_i32p),
                ("n_pred", C.c_int32), ("n_gt", C.c_int32), ("n_cand", C.c_int32), ("ov", C.c_void_p)]


class MatchArgs(C.Structure):                         # vrd_match_args
    _fields_ = [("pred_first", c_i32p), ("cand_first", c_i32p), ("cand", c_i32p), ("ov", C.c_void_p),
                ("n_videos", C.c_int32), ("n_pred", C.c_int32), ("n_cand", C.c_int32), ("n_gt", C.c_int32),
                ("threshold", C.c_double), ("detected", c_u8p), ("hit", c_i32p)]


class ProposalArgs(C.Structure):                      # vrd_proposal_args
    _fields_ = [("boxes", c_f32p), ("rows", C.c_int64), ("trk", C.c_void_p), ("video_max", c_f32p), ("trk_first", c_i32p),
                ("tri_first", C.c_void_p), ("cand_first", C.c_void_p), ("cand_s", c_i32p), ("cand_o", c_i32p),
                ("stride_offset", c_i32p), ("n_videos", C.c_int32), ("n_trk", C.c_int32), ("n_tri", C.c_int64),
                ("n_cand", C.c_int64), ("feat_stride", C.c_int32), ("min_frames", C.c_int32), ("threshold", C.c_double),
                ("trk_err", c_u8p), ("shadow", c_u8p), ("dropped", c_u8p), ("s_row", C.c_void_p), ("o_row", C.c_void_p),
                ("lens", c_i32p), ("kept_s", c_i32p), ("kept_o", c_i32p), ("count", c_i32p), ("video_err", c_i32p)]


class AssembleArgs(C.Structure):
    _fields_ = [("streams", c_f32p), ("snippets", c_f32p), ("stream_row", C.c_void_p), ("lens", C.c_void_p),
                ("P", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("L", C.c_int32), ("piece", C.c_int32), ("reach", C.c_int32),
                ("out", c_f32p)]


_SIGNATURES = {
    "vrd_abi_version": (C.c_int, []),
    "vrd_last_error": (C.c_char_p, []),
    "vrd_f16_range_flag": (C.c_int, [C.POINTER(C.c_void_p)]),
    "vrd_prof_enable": (C.c_int, [C.c_int]),
    "vrd_prof_reset": (C.c_int, []),
    "vrd_prof_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                C.POINTER(C.c_double)]),
    "vrd_prof_read_skipped": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "vrd_prof_select": (C.c_int, [C.c_uint64]),
    "vrd_bct_to_btc": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int64, C.c_int, C.c_int, c_i32p,
                                 C.c_void_p]),
    "vrd_btc_to_bct": (C.c_int, [c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_void_p]),
    "vrd_pack_pairs": (C.c_int, [C.POINTER(PackArgs), C.c_void_p]),
    "vrd_gather_pairs": (C.c_int, [C.POINTER(GatherArgs), C.c_void_p]),
    "vrd_gather_train": (C.c_int, [C.POINTER(GatherTrainArgs), C.c_void_p]),
    "vrd_assemble_pairs": (C.c_int, [C.POINTER(AssembleArgs), C.c_void_p]),
    "vrd_split_weight": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, c_f32p,
                                   C.c_void_p]),
    "vrd_split_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vrd_gemm": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "vrd_gemm_family": (C.c_int, [C.POINTER(GemmArgs)]),
    "vrd_gemm_batch": (C.c_int, [C.POINTER(GemmArgs), C.c_int, C.c_void_p]),
    "vrd_row_blocks": (C.c_int, [c_u8p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrd_conv_ln": (C.c_int, [C.POINTER(ConvLnArgs), C.c_void_p]),
    "vrd_layernorm": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, c_f32p, C.c_int,
                                c_f32p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    # position rows from per-sequence tables (pos_table, ld_pos, pos_rows, pos_first, mask, segs or NULL, T)
    "vrd_layernorm_pos": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, c_f32p, C.c_int,
                                    c_f32p, C.c_int64, C.c_int64, c_i32p, c_u8p, C.POINTER(RowSegs), C.c_int, C.c_int, C.c_void_p]),
    "vrd_position_rows": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, C.c_int64, C.c_int64, c_i32p, c_u8p,
                                    C.POINTER(RowSegs), C.c_int, C.c_int, C.c_void_p]),
    "vrd_dwconv_ln": (C.c_int, [C.POINTER(DwconvLnArgs), C.c_void_p]),
    "vrd_dwconv_ln_multi": (C.c_int, [C.POINTER(DwconvLnMultiArgs), C.c_void_p]),
    "vrd_local_attn": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_u8p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, c_f32p, C.c_int64, C.c_int, C.c_void_p]),
    "vrd_local_attn_segs": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_u8p, c_f32p, C.POINTER(RowSegs), C.c_int, C.c_int,
                                      C.c_int, c_f32p, C.c_int64, C.c_int, C.c_void_p]),
    "vrd_attention": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_u8p, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "vrd_attention_pair": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_u8p, c_u8p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "vrd_attention_pair_segs": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_u8p, c_u8p, C.POINTER(RowSegs),
                                          C.POINTER(RowSegs), C.c_int, C.c_int, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                          C.c_int]),
    "vrd_maxpool_mask": (C.c_int, [c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, c_u8p, c_f32p, C.c_int64, c_u8p,
                                   C.c_void_p]),
    "vrd_mask_head": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_float, c_f32p, C.c_void_p]),
    "vrd_postprocess": (C.c_int, [c_f32p, c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_i32p,
                                  c_i32p, c_i32p, C.c_void_p]),
    "vrd_select_triplets": (C.c_int, [C.POINTER(SelectArgs), C.c_void_p]),
    # ---- relation scoring (csrc/vrd_score.hip; vrdone_amd/evaluate.py DeviceRelationScorer)
    "vrd_relation_viou": (C.c_int, [C.POINTER(ViouArgs), C.c_void_p]),
    "vrd_match_relations": (C.c_int, [C.POINTER(MatchArgs), C.c_void_p]),
    # ---- eval proposals (csrc/vrd_proposals.hip; vrdone_amd/proposals.py prepare_test_videos)
    "vrd_proposal_clamp": (C.c_int, [C.POINTER(ProposalArgs), C.c_void_p]),
    "vrd_proposal_shadow": (C.c_int, [C.POINTER(ProposalArgs), C.c_void_p]),
    "vrd_proposal_walk": (C.c_int, [C.POINTER(ProposalArgs), C.c_void_p]),
    "vrd_proposal_pairs": (C.c_int, [C.POINTER(ProposalArgs), C.c_void_p]),
    # ---- backward kernels (training step)
    "vrd_gemm_wgrad": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                 c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int]),
    "vrd_gemm_wgrad_x3": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                    c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p, C.c_int]),
    "vrd_gemm_wgrad_x3_plan": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                         c_f32p, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    "vrd_scratch_required": (C.c_int, [C.POINTER(C.c_int64)]),
    "vrd_absmax_scale": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, C.c_void_p]),
    "vrd_dwconv_wgrad": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, c_u8p, C.c_int64,
                                   C.c_int, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int]),
    "vrd_colsum": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_u8p, c_f32p,
                             C.c_int64, C.c_int, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int]),
    "vrd_rowcol_scale": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, c_f32p, c_u8p, c_f32p, C.c_int64, C.c_int,
                                   c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_void_p]),
    "vrd_activation": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int64, C.c_int, C.c_int, c_f32p, C.c_int64, C.c_void_p]),
    "vrd_layernorm_bwd": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int64, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p,
                                    C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int]),
    "vrd_dwconv_bwd": (C.c_int, [C.POINTER(DwconvBwdArgs), C.c_void_p]),
    "vrd_local_attn_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, c_f32p, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    # ---- training dropout (csrc/vrd_dropout.hip, vrd_local_attn_bwd.hip; host mirror vrdone_amd/dropout.py): seed = a 64-bit word on the device
    "vrd_dropout_mask": (C.c_int, [C.c_void_p, C.c_uint, C.c_int64, C.c_int64, C.c_float, c_u8p, C.c_void_p]),
    "vrd_dropout_rows": (C.c_int, [c_f32p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_uint, C.c_int64, C.c_float, c_f32p, C.c_int64,
                                   C.c_void_p]),
    "vrd_local_attn_drop": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_u8p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_uint, C.c_int64, C.c_float, c_f32p, C.c_int64, C.c_void_p]),
    "vrd_local_attn_drop_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, c_f32p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint, C.c_int64, C.c_float, c_f32p, c_f32p, c_f32p,
                                          C.c_int64, c_f32p, C.c_void_p]),
    "vrd_attn_bwd_probs": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_void_p]),
    "vrd_bmm": (C.c_int, [C.POINTER(BmmArgs), C.c_void_p]),
    # the flash pair of a training step (vrd_attn_bwd.hip): head_dim 32 or 64, any other value is refused by name
    "vrd_attention_bwd": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_u8p, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_void_p]),
    "vrd_attention_rows": (C.c_int, [c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "vrd_assign": (C.c_int, [c_f32p, C.c_int64, c_i32p, c_i32p, C.c_int, C.c_int, c_i32p, C.c_void_p]),
    "vrd_assign_wave": (C.c_int, [c_f32p, C.c_int64, c_i32p, c_i32p, C.c_int, C.c_int, c_i32p, C.c_void_p]),
    "vrd_ema_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32p, c_i32p, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    # ---- gradient-norm clip + AdamW over pointer tables (csrc/vrd_optim.hip; vrdone_amd/optim.py)
    "vrd_grad_sumsq": (C.c_int, [C.c_void_p, C.c_void_p, c_i32p, c_i32p, c_i32p, C.c_int, C.c_void_p, C.c_void_p]),
    "vrd_grad_norm_finish": (C.c_int, [C.c_void_p, C.c_int, C.c_float, c_f32p, C.c_void_p]),
    "vrd_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i32p, c_i32p, c_f32p, C.c_int, c_i32p,
                                 c_i32p, C.c_int, c_f32p, C.c_void_p]),
    "vrd_scale_tensors": (C.c_int, [C.c_void_p, C.c_void_p, c_i32p, c_i32p, c_i32p, C.c_int, c_f32p, C.c_void_p]),
    "vrd_attn_bwd_softmax": (C.c_int, [c_f32p, c_f32p, c_u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vrd_criterion_costs": (C.c_int, [C.c_void_p, c_f32p, C.c_void_p]),
    "vrd_criterion_losses": (C.c_int, [C.c_void_p, c_i32p, c_f32p, C.c_float, c_f32p, C.c_void_p]),
    "vrd_criterion_backward": (C.c_int, [C.c_void_p, c_i32p, c_f32p, C.c_float, c_f32p, c_f32p, C.c_void_p, C.c_void_p]),
    "vrd_maxpool_bwd": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, c_u8p, c_f32p, C.c_int64,
                                  C.c_void_p]),
    # ---- the sequence-walking backward kernels over a ragged row space (vrd_row_segs): a training step in the row space
    "vrd_local_attn_bwd_segs": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, c_u8p, c_f32p, C.POINTER(RowSegs),
                                          C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_void_p]),
    "vrd_dwconv_bwd_segs": (C.c_int, [C.POINTER(DwconvBwdArgs), C.POINTER(RowSegs), C.c_void_p]),
    "vrd_dwconv_wgrad_segs": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(RowSegs), c_u8p,
                                        C.c_int, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_void_p, C.c_int]),
    "vrd_maxpool_bwd_segs": (C.c_int, [c_f32p, C.c_int64, c_f32p, C.c_int64, C.POINTER(RowSegs), C.c_int, c_u8p, c_f32p, C.c_int64,
                                       C.c_void_p]),
}

ABI_VERSION = 37
WGRAD_WAVE, WGRAD_LDS128, WGRAD_LDS256 = 0, 1, 2      # VRD_WGRAD_*: plan[0] of vrd_gemm_wgrad_x3_plan
WGRAD_PLAN_INTS = 7                                   # (form, vec, tiles, chunk, chunks, tile_partials, total_floats)

# `flags` of the parameter-gradient entry points (include/vrdone_hip.h): bit-reproducible sums, no float atomics; such a call
# fails with ERR_SCRATCH (before any launch) when its scratch is short, and lib.vrd_scratch_required() says how many floats it needs
DETERMINISTIC = 1
ERR_SCRATCH = -3


class HipLibraryError(RuntimeError):
    pass


# entry points whose trailing `flags` argument came with the deterministic mode: a caller written before it may leave it out (0)
_FLAGS_DEFAULT = ("vrd_gemm_wgrad_x3", "vrd_colsum", "vrd_dwconv_wgrad", "vrd_layernorm_bwd")


def _flags_default(fn):
    n = len(fn.argtypes)

    def call(*args):
        return fn(*args, 0) if len(args) == n - 1 else fn(*args)
    call.__name__, call.argtypes, call.restype = fn.__name__, fn.argtypes, fn.restype
    return call


def _load():
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} is missing: the HIP extension was not built "
            "(run `make -C vrdone_amd/csrc`); there is no CPU fallback for this path")
    # PyTorch ships its own libamdhip64.so: it has to be in the process first, so that the library binds to that runtime.
    # Loaded the other way round, the process holds two HIP runtimes and the library's launches fail on torch's memory
    # ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    for name in _FLAGS_DEFAULT:
        setattr(lib, name, _flags_default(getattr(lib, name)))
    got = lib.vrd_abi_version()
    if got != ABI_VERSION:
        raise HipLibraryError(f"libvrdone_hip.so ABI {got} != expected {ABI_VERSION}: rebuild it")
    return lib


lib = _load()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib.vrd_last_error().decode()}")


# tags of the f16 operand-range flag word (vrd_f16_range_flag; enum RangeTag of csrc/vrd_common.h): the entry points that OR each
# bit.  A value x reports from |x| >= 4095 on (|x * 2^4| >= 65520 rounds to hi = inf); |x| < 4094 is the documented safe bound.
RANGE_TAGS = {1: "boundary tensors (vrd_bct_to_btc / vrd_pack_pairs / vrd_gather_pairs / vrd_gather_train)",
              2: "vrd_layernorm / vrd_layernorm_pos / vrd_position_rows / vrd_conv_ln / vrd_dwconv_ln_multi outputs",
              4: "vrd_dwconv_ln outputs",
              8: "pair-row outputs of vrd_gemm / vrd_gemm_batch",
              16: "f32 rows split while staged (vrd_gemm / vrd_gemm_batch, vrd_attention_rows, vrd_attention_bwd)",
              32: "pair-row outputs of vrd_local_attn / vrd_local_attn_segs / vrd_attention",
              64: "other"}


def prof_enable(on=True):
    check(lib.vrd_prof_enable(1 if on else 0), "vrd_prof_enable")


def prof_select(families=None):
    """Record events only for the named kernel families (None = all)."""
    mask = (1 << 64) - 1 if families is None else sum(1 << KERNEL_NAMES.index(f) for f in families)
    check(lib.vrd_prof_select(mask), "vrd_prof_select")


def prof_reset():
    check(lib.vrd_prof_reset(), "vrd_prof_reset")


def prof_read():
    """{family: dict(ms=, launches=, flops=, bytes=, flops_skipped=)} of everything recorded since the last reset.
    flops = what the launches were sized for (2*M*N*K); flops_skipped = the part padding maps made the kernel skip."""
    out = {}
    for kid, name in enumerate(KERNEL_NAMES):
        ms, n, fl, by, sk = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        check(lib.vrd_prof_read(kid, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "vrd_prof_read")
        check(lib.vrd_prof_read_skipped(kid, C.byref(sk)), "vrd_prof_read_skipped")
        out[name] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value, "flops_skipped": sk.value}
    return out
