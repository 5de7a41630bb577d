"""The table of tools/mutants.py: one value-changing edit per row and the operator checks that must notice it.

A row: id | file (under cistgcn_amd/csrc) | old text | new text | count (how often the old text occurs; every occurrence is edited) |
checks: "module.function" or ("module.function", args after the device, kwargs) of tests/, or one of the drivers below (a check that the
tests call once per case, here in a loop over the cases).  Edits change values only - a constant, an operator, a dropped or doubled
addend, a swapped operand or salt, a branch taken the other way - and never an index past a 3 x 3 matrix or a two-entry table, a bound,
a pointer, a launch geometry or a barrier: no row can read or write out of range or hang.  tests/MUTANTS.md has the outcomes."""


# ---- drivers: checks that take a case ----------------------------------------------------------------------------------------------
def attack_steps(device):
    import attack_checks as A
    for shape in A.STEP_SHAPES:
        for mode in A.STEP_MODES:
            for mask in A.STEP_MASKS:
                A.check_attack_step_synthetic(device, shape, mode, mask)


def attack_mpjpe(device):
    import attack_checks as A
    for shape in A.MPJPE_SHAPES:
        A.check_mpjpe_per_sample(device, *shape)


def attack_metrics(device):
    import attack_metrics_checks as AM
    for case in AM.CASES:
        for key in AM.KEYS:
            AM.check_against_fixture(device, case, key)
    for shape in AM.SHAPES:
        AM.check_shape(device, shape)


def eval_metrics(device):
    import metrics_checks as M
    for case in M.CASES:
        for mode in M.MODES:
            for metric in M.METRICS:
                M.check_against_fixture(device, case, mode, metric)


def losses(device):
    import losses_checks as LC
    for case in LC.cases():
        LC.check_against_fixture(device, case)
    for shape in LC.loop_shapes():
        for kind in LC.KINDS:
            for source in LC.SOURCES:
                LC.check_shape(device, shape, kind, source)


def kinematics(device):
    import kinematics_checks as KC
    for case in KC.CASES:
        KC.check_fk_fixture(device, case)
    for shape in KC.fk_shapes():
        KC.check_fk_shape(device, shape)
    for shape in KC.GATHER_SHAPES:
        KC.check_gather_shape(device, shape)


def robustness(device):
    import robustness_checks as RC
    for case in RC.CASES:
        RC.check_against_fixture(device, case)
    for shape in RC.SHAPES:
        RC.check_shape(device, shape)


def augmentation(device):
    import test_environment as E
    E.check_augmentation_golden(device)
    E.check_augmentation_noise_inversion_golden(device)
    E.check_augmentation_vs_oracle(device, B=3, L=20, J=7, input_n=12)


def block_mid(device):
    import block_mid_checks as C
    for mode in C.MODES:
        C.check_operator(device, "six", mode)


def stgcn_tiles(device):
    """tile and matrix-core kernels of csrc/stgcn_domain.hip and csrc/stgcn_domain_mfma.hip (the plane generation pinned off)"""
    import checks
    import loop_shapes as L
    checks.check_stgcn_domain(device, shapes=((3, 10, 8, 5, 7), (2, 3, 3, 6, 9), (2, 18, 16, 5, 7)))
    checks.check_stgcn_domain(device, shapes=L.STGCN_TILE[:1], planes=None)
    checks.check_stgcn_domain(device, shapes=L.STGCN_MFMA[:1], planes=None)


def stgcn_planes(device):
    import checks
    checks.check_stgcn_domain(device, shapes=checks.PLANE_SHAPES[-2:], planes=True)


EDGES, TIES, DROPOUT = "audit_checks.check_contract_edges", "audit_checks.check_context_ties", ("checks.check_dropout", (), {"mask": True})
# one check per family, so that the table shows every family killing the row on its own (the names of audit_checks.LOW_VARIANCE)
LOWVAR = [("audit_checks.check_low_variance", (family,)) for family in (
    "norm_act", "norm_act_many", "dstd_tail", "map2adj_tail", "block_input", "gate_head", "block_mid", "tower_maps", "tower_collapse", "context_heads")]
ADAM = ["checks.check_flat_adam", "glue_checks.check_flat_adam"]
ADAM_CLIP = "glue_checks.check_flat_adam_clip"


STATS_DEGENERATE = ["checks.check_stage_kernels", "glue_checks.check_dstd_stats", "degenerate_checks.check_dstd_stats_degenerate"]
BIN_DEGENERATE = ["checks.check_block_input", "degenerate_checks.check_block_input_degenerate"]

FPN = ("checks.check_dilated_convs", (), {"shapes": ((3, 6, 5, 4, 6), (2, 5, 4, 10, 7))})

def off_centre(name):
    return ("off_centre_checks.check_off_centre", (name,))


ROWS = [
    # ---- the ten trials of the audit (one edit each: the two-place edits of the issue are two rows) ----
    dict(id="contract-bias-in-every-split", file="contract.hip", count=2, old="(row_ok && bias != nullptr && sk == 0)", new="(row_ok && bias != nullptr)", checks=[EDGES]),
    dict(id="ctx-last-argmax-in-slice", file="context_heads.hip", old="if (z0 > best) { best = z0; arg = p; }", new="if (z0 >= best) { best = z0; arg = p; }", checks=[TIES]),
    dict(id="ctx-last-argmax-in-merge", file="context_heads.hip", old="if (j == 0 || v > best) { best = v;", new="if (j == 0 || v >= best) { best = v;", checks=[TIES]),
    dict(id="bn-eps-dropped-train", file="cg_bn.h", old="return (float)(1.0 / sqrt(var + (double)eps));", new="return (float)(1.0 / sqrt(var + 0.0 * (double)eps));", checks=LOWVAR),
    dict(id="bn-eps-dropped-eval", file="cg_bn.h", old="return 1.0f / sqrtf(running_var + eps);", new="return 1.0f / sqrtf(running_var + 0.f * eps);", checks=LOWVAR),
    dict(id="dropout-mask-period-16384", file="cg_common.h", old="unsigned long long z = quad + seed *", new="unsigned long long z = (quad & 0xFFF) + seed *", checks=[DROPOUT]),
    dict(id="dropout-draws-overlap", file="cg_common.h", old="(uint32_t)(bits >> (16 * j))", new="(uint32_t)(bits >> (8 * j))", checks=[DROPOUT]),
    dict(id="bn-biased-running-var", file="cg_bn.h", old="const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;", new="const double unb = var;", checks=["checks.check_norm_act", "checks.check_block_input"]),
    dict(id="bn-no-batch-count", file="cg_bn.h", old="*num_batches_tracked += 1;", new="*num_batches_tracked += 0;", checks=["checks.check_norm_act", "checks.check_block_input"]),
    dict(id="adam-weight-decay-dropped", file="optim.hip", old="gi += wd * pi;", new="gi += 0.f * pi;", checks=ADAM),
    dict(id="adam-decoupled-decay", file="optim.hip", old="const float pi = p[i];\n    gi += wd * pi;", new="const float pi = p[i] * (1.f - lr * wd);", checks=ADAM),
    dict(id="adam-eps-inside-sqrt", file="optim.hip", old="sqrtf(vi) / bc2_sqrt + eps;", new="sqrtf(vi + eps) / bc2_sqrt;", checks=ADAM),
    dict(id="adam-second-moment-raw-grad", file="optim.hip", old="(1.f - b2) * gi * gi;", new="(1.f - b2) * (g[i] * gscale) * (g[i] * gscale);", checks=ADAM),
    dict(id="adam-clip-swallows-nan", file="optim.hip", old="gi = gi < -clip ? -clip : (gi > clip ? clip : gi);", new="gi = fminf(fmaxf(gi, -clip), clip);", checks=ADAM + [ADAM_CLIP]),
    dict(id="adam-clip-before-scale", file="optim.hip", old="float gi = g[i] * gscale;\n    if (clip > 0.f) gi = gi < -clip ? -clip : (gi > clip ? clip : gi);",
         new="float gi = g[i];\n    if (clip > 0.f) gi = gi < -clip ? -clip : (gi > clip ? clip : gi);\n    gi *= gscale;", checks=ADAM + [ADAM_CLIP]),
    # ---- a float64-per-element BatchNorm sum demoted to float32 squares or a float32 quad: the family's own check first (it must pass), then its off-centre case ----
    dict(id="rows-stats-f32-quad", file="rowops.hip",
         old="s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);\n      q += ((double)v[0] * v[0] + (double)v[1] * v[1]) + ((double)v[2] * v[2] + (double)v[3] * v[3]);",
         new="s += (double)((v[0] + v[1]) + (v[2] + v[3]));\n      q += (double)((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));",
         checks=["checks.check_norm_act", off_centre("norm_act")]),
    dict(id="contract-stats-f32-square", file="contract.hip", count=2, old="s += (double)v; q += (double)v * (double)v;", new="s += (double)v; q += (double)(v * v);",
         checks=["checks.check_contract", off_centre("contract_stats")]),
    dict(id="contract-stream-stats-f32-quad", file="contract.hip", old="double s2 = ok ? ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w) : 0.0;",
         new="double s2 = ok ? (double)((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w)) : 0.0;", checks=["checks.check_contract_stream", off_centre("contract_stats")]),
    dict(id="stgcn-tile-stats-f32-square", file="stgcn_domain.hip", old="s += (double)v; sq += (double)v * (double)v;", new="s += (double)v; sq += (double)(v * v);",
         checks=["mutants_table.stgcn_tiles", off_centre("stgcn_stats_tile")]),
    dict(id="dstd-f1-stats-f32-square", file="dstd_tail.hip", old="const double z = (double)(wv * xv[j]);\n          s += z; q += z * z; ",
         new="const float zf = wv * xv[j];\n          const double z = (double)zf;\n          s += z; q += (double)(zf * zf); ", checks=["checks.check_dstd_tail", off_centre("dstd_tail")]),
    dict(id="collapse-rows-stats-f32-square", file="collapse_rows.hip", old="{ const double y = (double)sY[o * 33 + v]; s1 += y; s2 += y * y; }",
         new="{ const float y = sY[o * 33 + v]; s1 += (double)y; s2 += (double)(y * y); }", checks=["checks.check_collapse_rows", off_centre("collapse_rows_stats")]),
    # ---- two rows for every other source ----
    dict(id="attack-momentum-factor-dropped", file="attack.hip", old="const float m = a.mu * a.g[base + i];", new="const float m = a.g[base + i];", checks=["mutants_table.attack_steps"]),
    dict(id="attack-sample-grad-N-dropped", file="attack.hip", old="w[blockIdx.y] / ((float)N * n)", new="w[blockIdx.y] / n", checks=["mutants_table.attack_mpjpe"]),
    dict(id="am-mse-divisor", file="attack_metrics.hip", old="(float)(s[CG_AM_S_SE] / (3.0 * den));", new="(float)(s[CG_AM_S_SE] / (2.0 * den));", checks=["mutants_table.attack_metrics"]),
    dict(id="am-ks-signed", file="attack_metrics.hip", old="cg_wave_allmax(fabs((double)cum) / (double)hist_n / width);", new="cg_wave_allmax(((double)cum) / (double)hist_n / width);", checks=["mutants_table.attack_metrics"]),
    dict(id="block-input-biased-std", file="block_input.hip", old="cs[c] = sqrtf(q / (float)(T * V - 1));", new="cs[c] = sqrtf(q / (float)(T * V));", checks=["checks.check_block_input"]),
    dict(id="block-input-grad-V-dropped", file="block_input.hip", old="const float g0 = sg[0] / (float)(C * T * V);", new="const float g0 = sg[0] / (float)(C * T);", checks=["checks.check_block_input"]),
    dict(id="block-mid-backward-mask-dropped", file="block_mid.hip", old="const float g = (neg ? alpha * dh : dh) * keep;", new="const float g = (neg ? alpha * dh : dh);", checks=["mutants_table.block_mid"]),
    dict(id="block-mid-forward-slope-dropped", file="block_mid.hip", old="h = it.alpha ? (u > 0.f ? u : it.alpha[0] * u) : u;", new="h = it.alpha ? (u > 0.f ? u : u) : u;", checks=["mutants_table.block_mid"]),
    dict(id="collapse-backward-slope-dropped", file="collapse_rows.hip", old="const float gh = u > 0.f ? dh : ta * dh;", new="const float gh = dh;", checks=["checks.check_tower_collapse"]),
    dict(id="collapse-transform-beta-sign", file="collapse_rows.hip", old="f.x0[s] = cg_prelu((f.x0[s] - k4.x) * k4.y + k4.z, in_alpha);", new="f.x0[s] = cg_prelu((f.x0[s] - k4.x) * k4.y - k4.z, in_alpha);", checks=["checks.check_tower_collapse"]),
    dict(id="dstd-gate-factor-dropped", file="dstd_tail.hip", old="v[j] = h[j] * gate + rv[j];", new="v[j] = h[j] + rv[j];", checks=["checks.check_dstd_tail"]),
    dict(id="dstd-keep-factor-squared", file="dstd_tail.hip", old="? 1.0f / (1.0f - hot.drop_p) : 1.f;", new="? 1.0f / ((1.0f - hot.drop_p) * (1.0f - hot.drop_p)) : 1.f;", checks=["checks.check_dstd_tail"]),
    dict(id="dstd-salts-swapped", file="dstd_tail.hip", old="return cg_drop_scale(t.drop_p, seed, t.salt[i],", new="return cg_drop_scale(t.drop_p, seed, t.salt[1 - i],", checks=["checks.check_dstd_tail"]),
    dict(id="em-frame-ramp", file="eval_metrics.hip", old="return (double)((float)(t + 1) / (float)To);", new="return (double)((float)t / (float)To);", checks=["mutants_table.eval_metrics"]),
    dict(id="em-bone-joint-count-swapped", file="eval_metrics.hip", old="(double)(bone ? a.Nb : a.J)", new="(double)(bone ? a.J : a.Nb)", checks=["mutants_table.eval_metrics"]),
    dict(id="fpn-bias-dropped", file="fpn_conv.hip", old="const float bias = t.bias[di] ? t.bias[di][o] : 0.f;", new="const float bias = 0.f;", checks=[FPN]),
    dict(id="fpn-bias-grad-doubled", file="fpn_conv.hip", old="if (kt0 == 0) { if (ot0) bsum1 += bs0; else bsum += bs0; }", new="if (kt0 == 0) { if (ot0) bsum1 += bs0; else bsum += bs0 + bs0; }", checks=[FPN]),
    dict(id="gate-forward-salt-swapped", file="gate_head.hip", old="const float keep = drop ? cg_drop_scale(t.drop_p, seed, p.salt2,", new="const float keep = drop ? cg_drop_scale(t.drop_p, seed, p.salt3,", checks=["checks.check_gate_head"]),
    dict(id="gate-slope-of-the-other-prelu", file="gate_head.hip", old="const float v = uu > 0.f ? uu : p.alpha3[0] * uu;", new="const float v = uu > 0.f ? uu : p.alpha2[0] * uu;", checks=["checks.check_gate_head"]),
    dict(id="aug-flip-sign", file="input_pipeline.hip", old="if (par[a] != 0.f) s[e] = c[a] - (s[e] - c[a]);", new="if (par[a] != 0.f) s[e] = c[a] + (s[e] - c[a]);", checks=["mutants_table.augmentation"]),
    dict(id="perturb-ramp-n-for-n-1", file="input_pipeline.hip", old="return n > 1 ? (float)(t - s0) / (float)(n - 1) : 0.f;", new="return n > 1 ? (float)(t - s0) / (float)n : 0.f;", checks=["mutants_table.robustness"]),
    dict(id="fk-parent-quirk-fixed", file="kinematics.hip", old="(CONV == CG_FK_SMPL ? par >= 0 : par > 0)", new="(CONV == CG_FK_SMPL ? par >= 0 : par >= 0)", checks=["mutants_table.kinematics"]),
    dict(id="fk-rodrigues-transposed", file="kinematics.hip", old="R[3 * i + j] = ((i == j ? 1.0 : 0.0) + sn * K[i][j]) + c1 * kk;", new="R[3 * i + j] = ((i == j ? 1.0 : 0.0) + sn * K[j][i]) + c1 * kk;", checks=["mutants_table.kinematics"]),
    dict(id="loss-smooth-l1-offset-dropped", file="losses.hip", old="return a < 1.f ? 0.5f * d * d : a - 0.5f; }", new="return a < 1.f ? 0.5f * d * d : a; }", checks=["mutants_table.losses"]),
    dict(id="loss-rmpjpe-grad-factor-2", file="losses.hip", old="k0 = M > 0.f ? k0 / (2.0 * sqrt((double)M)) : 0.0;", new="k0 = M > 0.f ? k0 / sqrt((double)M) : 0.0;", checks=["mutants_table.losses"]),
    dict(id="adj-backward-mask-dropped", file="map2adj_tail.hip", old="gv[q] = in ? (upre > 0.f ? c[q] : alpha * c[q]) * kv[q] : 0.f;", new="gv[q] = in ? (upre > 0.f ? c[q] : alpha * c[q]) : 0.f;", checks=["checks.check_map2adj_tail"]),
    dict(id="adj-beta-dropped-in-backward-replay", file="map2adj_tail.hip", old="const float h = cg_prelu((gam * bv[s] + bet) * keep[s], alpha);", new="const float h = cg_prelu((gam * bv[s]) * keep[s], alpha);", checks=["checks.check_map2adj_tail"]),
    dict(id="rows-add-post-dropped", file="rowops.hip", old="if (a.add && a.add_post) u += ad;", new="if (a.add && a.add_post) u += 0.f * ad;", checks=["checks.check_norm_act"]),
    dict(id="rows-pre-factor-dropped-backward", file="rowops.hip", count=2, old="      const float w = a.pre ? a.pre[(long long)b * C + c] : 1.f;", new="      const float w = 1.f;", checks=["checks.check_norm_act"]),
    dict(id="stats-biased-std", file="stages.hip", old="cs[c] = sqrtf(q / (float)(T * V - 1));", new="cs[c] = sqrtf(q / (float)(T * V));", checks=["checks.check_stage_kernels"]),
    dict(id="se-gate-sigmoid-sign", file="stages.hip", old="gate[(long long)b * C + c] = 1.f / (1.f + expf(-s));", new="gate[(long long)b * C + c] = 1.f / (1.f + expf(s));", checks=["checks.check_reduce_and_gate"]),
    dict(id="stgcn-tile-bias-dropped", file="stgcn_domain.hip", old="const float bv = bias ? bias[co] : 0.f;", new="const float bv = 0.f;", checks=["mutants_table.stgcn_tiles"]),
    dict(id="stgcn-mfma1-bias-sign", file="stgcn_domain.hip", old="const float v = ok ? acc[q] + (bias ? bias[co] : 0.f) : 0.f;", new="const float v = ok ? acc[q] - (bias ? bias[co] : 0.f) : 0.f;", checks=["mutants_table.stgcn_tiles", ("checks.check_stgcn_domain", (), {"shapes": ((2, 128, 128, 3, 4),)}), "audit_checks.check_stgcn_wide_rows"]),
    dict(id="stgcn-mfma-bias-dropped", file="stgcn_domain_mfma.hip", old="const float bv = (cok && bias) ? bias[co] : 0.f;", new="const float bv = 0.f;", checks=["mutants_table.stgcn_tiles"]),
    dict(id="stgcn-mfma-bias-grad-doubled", file="stgcn_domain_mfma.hip", old="if (ntl == 0) bacc[u] += bs;", new="if (ntl == 0) bacc[u] += bs + bs;", checks=["mutants_table.stgcn_tiles"]),
    dict(id="stgcn-planes-bias-dropped", file="stgcn_domain_planes.hip", old="bv[r] = (bias && co < g.Cout) ? bias[co] : 0.f;", new="bv[r] = 0.f;", checks=["mutants_table.stgcn_planes"]),
    dict(id="stgcn-planes-bias-grad-doubled", file="stgcn_domain_planes.hip", old="for (int i = 0; i < 4; ++i) dbw[i] += dbp[i];", new="for (int i = 0; i < 4; ++i) dbw[i] += dbp[i] + dbp[i];", checks=["mutants_table.stgcn_planes"]),
    dict(id="maps-bias-dropped", file="tower_maps.hip", old="sBias[r] = (m < t.M[i] && t.bias[i]) ? t.bias[i][m] : 0.f;", new="sBias[r] = 0.f;", checks=["checks.check_pointwise_maps", "checks.check_tower_maps"]),
    dict(id="maps-bn-backward-mean-of-g", file="tower_maps.hip", old="k_m1[r] = (float)(t.bn_red[i][2 * m] / cnt);", new="k_m1[r] = (float)(t.bn_red[i][2 * m] / (cnt - 1.0));", checks=["checks.check_tower_maps"]),
    dict(id="maps-backward-prelu-ge", file="tower_maps.hip", old="const float gu = u > 0.f ? dbuf[4 * r + j] : k_alpha[r] * dbuf[4 * r + j];", new="const float gu = u >= 0.f ? dbuf[4 * r + j] : k_alpha[r] * dbuf[4 * r + j];", checks=["checks.check_tower_maps"]),
    # ---- constant rows, channels and samples in the block statistics: each zero-std mask removed, each mean of equal values put back to sum / n;
    #      the family's own check first (it must pass), then the degenerate case ----
    dict(id="stats-mask-std-of-channel-stds", file="stages.hip", old="const float ac = gS > 0.f ? gall", new="const float ac = true ? gall", checks=STATS_DEGENERATE),
    dict(id="stats-mask-channel-std", file="stages.hip", old="const float pc = cs[c] > 0.f ? ac", new="const float pc = true ? ac", checks=STATS_DEGENERATE),
    dict(id="stats-mask-std-of-row-stds", file="stages.hip", old="const float ar = tS[t] > 0.f ? g[2 + T + t]", new="const float ar = true ? g[2 + T + t]", checks=STATS_DEGENERATE),
    dict(id="stats-mask-row-std", file="stages.hip", old="const float pr = sct > 0.f ? ar", new="const float pr = true ? ar", checks=STATS_DEGENERATE),
    dict(id="stats-row-mean-plain-sum", file="stages.hip", old="if (cg_stats_group_sum(ne[k], lpr) == 0.f) m[k] = f[k];", new="if (cg_stats_group_sum(ne[k], lpr) < 0.f) m[k] = f[k];", checks=STATS_DEGENERATE),
    dict(id="stats-channel-mean-plain-sum", file="stages.hip", old="m = equal ? m0 : m / (float)T;", new="m = m / (float)T;", checks=STATS_DEGENERATE),
    dict(id="stats-mean-over-c-plain-sum", file="stages.hip", old="const float m = equal ? f0 : s / (float)C;", new="const float m = s / (float)C;", checks=STATS_DEGENERATE),
    dict(id="block-input-mask-std-of-channel-stds", file="block_input.hip", old="const float ac = gS > 0.f ? gall", new="const float ac = true ? gall", checks=BIN_DEGENERATE),
    dict(id="block-input-mask-channel-std", file="block_input.hip", old="const float pc = cs[c] > 0.f ? ac", new="const float pc = true ? ac", checks=BIN_DEGENERATE),
    dict(id="block-input-mask-std-of-row-stds", file="block_input.hip", old="const float ar = tS[k] > 0.f ? sg[2 + T + k]", new="const float ar = true ? sg[2 + T + k]", checks=BIN_DEGENERATE),
    dict(id="block-input-mask-row-std", file="block_input.hip", old="const float pr = sct > 0.f ? ar", new="const float pr = true ? ar", checks=BIN_DEGENERATE),
    dict(id="block-input-row-mean-plain-sum", file="block_input.hip", old="const float m = equal ? x0 : s / (float)t.V;", new="const float m = s / (float)t.V;", checks=BIN_DEGENERATE),
    dict(id="block-input-channel-mean-plain-sum", file="block_input.hip", old="m = equal ? m0 : m / (float)T;", new="m = m / (float)T;", checks=BIN_DEGENERATE),
    dict(id="block-input-mean-over-c-plain-sum", file="block_input.hip", old="const float m = equal ? f0 : s / (float)C;", new="const float m = s / (float)C;", checks=BIN_DEGENERATE),
]
