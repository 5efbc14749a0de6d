#!/usr/bin/env python3
"""Opcode ledger of k_ransac<64,16,6,true,true> (the benchmarked instantiation): every instruction of the compiler's
assembly is attributed to a PHASE of the kernel through its source line (-gline-tables-only: `.loc` directives name
the innermost inlined function's line), classified by opcode, and multiplied by how often its phase runs per launch
(the execution counts of the counting build, profiles/rNN_ransac_counts.json; without that file: static counts only).
Beside the VALU classes it reports what does not show in SQ_INSTS_VALU: s_nop (instructions and the idle cycles they
ask for) and s_waitcnt per phase, and for every 4-point loop body the VALU instructions that read the result of the
instruction immediately before them.

    tools/ransac_isa.py [profiles/r07_ransac_counts.json] [--src FILE] [--slp] [--sq FILE KEY] > profiles/r08_ransac_isa.txt
    (--src: another revision of ransac.hip, e.g. `git show HEAD~1:octreelib_amd/csrc/ransac.hip`, compiled against this
     tree's headers; --slp: without -fno-slp-vectorize, as revisions before round 8 were built; --sq: the measured
     SQ_INSTS_VALU to print beside the estimate, e.g. profiles/r08_sq_counters.json round8)

Phases (source line ranges of csrc/ransac.hip, found by the function / lambda they belong to):
    block     per block: descriptor and point prefetch, staging of the next block, uniforms of the bounds, reduction over
              the wave, winner, outputs, final mask
    fit       one exact plane fit of 64 hypotheses: positions, LDS gathers, plane_from_samples (the reference's f64
              sequence), the screen's constants                         runs: exact groups (group 0 + survivor batches)
    fit_cold  ... its branched-over fall-backs (true division, scaled square root, risky draws)   runs: ~never
    score     the exact count of 64 hypotheses: f32 screen + recount     runs: exact groups; its loop body per 4 points
    pre_fit   approximate f32 plane + bound of 3 x 64 hypotheses          runs: prescreen trios
    partition the two-stage count's setup: m1, the permuted copy of the points   runs: two-stage blocks
    stage1    widened count of a trio over the first m1 points            runs: trios of two-stage blocks; body per 4 points
    ring      undecided hypotheses -> the stage-2 ring in LDS             runs: trios of two-stage blocks
    stage2    one queued hypothesis per lane over the other points        runs: stage-2 passes; body per 4 points
    single    widened count of a trio over all points (blocks without two stages)   runs: their trios; body per 4 points
    queue     survivors -> LDS queue, the batches' bookkeeping            runs: prescreen trios / batches
"""
import collections, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "octreelib_amd", "csrc", "ransac.hip")
argv = sys.argv[1:]
SLP = "--slp" in argv
if SLP:
    argv.remove("--slp")
SQ = None
if "--sq" in argv:     # --sq profiles/rNN_sq_counters.json KEY: the measured VALU count to set the estimate against
    SQ = (argv[argv.index("--sq") + 1], argv[argv.index("--sq") + 2])
    del argv[argv.index("--sq"):argv.index("--sq") + 3]
if "--src" in argv:
    SRC = os.path.abspath(argv[argv.index("--src") + 1])
    del argv[argv.index("--src"):argv.index("--src") + 2]
KERNEL = r"^_ZN.*k_ransacILi64ELi16ELi6ELb1ELb1E.*:"

src_lines = open(SRC).read().split("\n")


def line_of(pattern, start=0):
    for i in range(start, len(src_lines)):
        if re.search(pattern, src_lines[i]):
            return i + 1
    raise SystemExit(f"ransac.hip: no line matches {pattern!r}")


# source line ranges -> phase
L = {
    "helpers_begin": 1,
    "plane_fit_begin": line_of(r"^__device__ __forceinline__ double div_by_small_int"),
    "plane_fit_end": line_of(r"^__device__ __forceinline__ double plane_distance"),
    "screen_group": line_of(r"^__device__ __forceinline__ void screen_group"),
    "prescreen_const": line_of(r"^struct PreConst"),
    "screen_ub": line_of(r"^__device__ __forceinline__ void screen_ub"),
    "kernel": line_of(r"^__global__ __launch_bounds__\(THREADS, (RS_MINWAVES|rs_minwaves\(THREADS, KT\))\) void k_ransac"),
}
L["shared_begin"] = line_of(r"^typedef float f4 ")
L["stage_local"] = line_of(r"^__device__ __forceinline__ void stage_local")
L["load_pos"] = line_of(r"auto load_pos = \[&\]", L["kernel"])
L["fit"] = line_of(r"auto fit = \[&\]", L["kernel"])
L["score"] = line_of(r"auto score = \[&\]", L["kernel"])
L["take"] = line_of(r"auto take = \[&\]", L["kernel"])
L["group0"] = line_of(r"---- group 0", L["kernel"])
L["prescreen"] = line_of(r"---- prescreen of the wave's later hypotheses", L["kernel"])
L["two_stage"] = line_of(r"---- the two-stage widened count", L["kernel"])
L["survive"] = line_of(r"auto survive = \[&\]", L["kernel"])
L["stage2"] = line_of(r"auto stage2 = \[&\]", L["kernel"])
L["pre_fit"] = line_of(r"auto prescreen = \[&\]", L["kernel"])
L["stage1"] = line_of(r"if \(two_stage\) \{   // \(wave-uniform\)", L["kernel"])
L["ring"] = line_of(r"screen_ub<\w+>\(ploc, m1", L["kernel"]) + 1
L["single"] = line_of(r"screen_ub<\w+>\(loc, n", L["kernel"])
L["trios"] = line_of(r"constexpr int PNH = ", L["kernel"])
L["survivors"] = line_of(r"---- the survivors \(in index order\)", L["kernel"])
L["tail"] = line_of(r"const uint32_t wbest = wave_max_u32\(best\);", L["kernel"])
L["kernel_end"] = line_of(r"^// A block with more than THREADS-1 points", L["kernel"])


COUNT_LOOPS = ("stage1", "stage2", "single")


def phase_of(line):
    """phase of a source line; None: a helper shared by several phases, "count": the widened count's loop - ONE function
    for stage 1, stage 2 and the single-stage count: the phase of the line it was inlined at decides"""
    # helpers shared by several phases (fma32, min3abs, the DPP reductions): the phase of the code around them
    if L["shared_begin"] <= line < L["stage_local"] - 4:
        return None
    if L["plane_fit_begin"] <= line < L["plane_fit_end"]:
        return "fit"
    if L["screen_group"] <= line < L["prescreen_const"]:
        # (round 8: score_pairs / push_bits, the body shared by both count loops, sit in front of screen_group)
        return "score"
    if L["prescreen_const"] <= line < L["screen_ub"]:
        return "block"          # prescreen_constants: once per block
    if L["screen_ub"] <= line < L["kernel"]:
        return "count"
    if L["load_pos"] <= line < L["score"]:
        return "fit"
    if L["score"] <= line < L["take"]:
        return "score"
    if L["take"] <= line < L["group0"]:
        return "fit"            # (take: per exact group)
    if L["group0"] <= line < L["prescreen"]:
        return "fit"
    if L["prescreen"] <= line < L["two_stage"]:
        return "block"
    if L["two_stage"] <= line < L["survive"]:
        return "partition"
    if L["survive"] <= line < L["stage2"]:
        return "queue"
    if L["stage2"] <= line < L["pre_fit"]:
        return "stage2"
    if L["pre_fit"] <= line < L["stage1"]:
        return "pre_fit"
    if L["stage1"] <= line < L["ring"]:
        return "stage1"
    if L["ring"] <= line < L["single"]:
        return "ring"
    if L["single"] <= line < L["trios"]:
        return "single"
    if L["trios"] <= line < L["tail"]:
        return "queue"
    return "block"


def phase_of_chain(lines):
    """lines: the source lines of a `.loc` and of the calls it was inlined through, innermost first"""
    count = False
    for line in lines:
        ph = phase_of(line)
        if ph == "count":
            count = True
        elif ph is not None:
            return (ph if ph in COUNT_LOOPS else "single") if count else ph
    return "single" if count else None


def opclass(op):
    if re.match(r"v_(add|mul|fma|fmac|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|max|min|trunc|floor|frexp).*_f64", op):
        return "f64 arithmetic"
    if re.match(r"v_(fma|fmac|mul|add|sub|subrev|pk_add|pk_mul|pk_fma|rsq|rcp|max|min|max3|min3|med3)_f32", op) or op.startswith("v_pk_"):
        return "f32 arithmetic"
    if op.startswith("v_cvt_"):
        return "v_cvt"
    if op.startswith("v_cmp") or op.startswith("v_cmpx"):
        return "v_cmp"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "v_mov"
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane") or "dpp" in op or op.startswith("v_permlane"):
        return "cross-lane"
    if re.match(r"v_(alignbit|bcnt|bfi|bfe|and|or|xor|not|lshl|lshr|ashr|perm)", op):
        return "bit ops (inlier bits, sign, bytes)"
    if re.match(r"v_(add|sub|subrev|mad|mul|lshl_add|add_lshl|lshl_or|and_or|min|max|mbcnt|addc|subb)", op):
        return "integer / address"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"):
        return "VMEM"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt") or op.startswith("s_barrier"):
        return "s_waitcnt / s_barrier"
    if op.startswith("s_"):
        return "SALU"
    return "other"


with tempfile.TemporaryDirectory() as d:
    out = os.path.join(d, "ransac.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off",
                    *([] if SLP else ["-fno-slp-vectorize"]), "-gline-tables-only", f"-I{ROOT}/include",
                    f"-I{ROOT}/octreelib_amd/csrc", "-S", "--cuda-device-only", SRC, "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    asm = open(out).read().split("\n")
start = next(i for i, l in enumerate(asm) if re.match(KERNEL, l))
end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
body = asm[start:end]

# instructions with (phase, class, cold?).  Cold = inside a region that a branch skips and that holds the true
# division / scaled square root / exact sample index sequences (never taken on sane data).
COLD = re.compile(r"v_div_scale|v_div_fmas|v_div_fixup|v_ldexp_f64|v_cmp_class|v_frexp|v_cvt_i32_f64|v_sqrt_f64")
blocks, cur = [], []
for l in body:
    if re.match(r"^\.LBB\d+_\d+:", l):
        blocks.append(cur)
        cur = []
    cur.append(l)
blocks.append(cur)
counts = collections.defaultdict(collections.Counter)   # (phase, in a 4-point loop body?) -> class -> static count
nop_cycles = collections.Counter()                      # (phase, in a 4-point loop body?) -> idle cycles s_nop asks for
bodies = []                                             # the 4-point loop bodies: (label, phase, VALU, s_nop, dependent)


def vregs(tok):
    tok = tok.strip().lstrip("-").strip("|")
    m = re.match(r"^v(\d+)$", tok)
    if m:
        return {int(m.group(1))}
    m = re.match(r"^v\[(\d+):(\d+)\]$", tok)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


LOC = re.compile(r"(?:^|[\s/\[])" + re.escape(os.path.basename(SRC)) + r":(\d+):\d+")
cur_phase = "block"
for b in blocks:
    cold = any(COLD.search(l) for l in b)
    in_loop4 = sum("ds_read_b128" in l for l in b) >= 4 and any("v_alignbit_b32" in l for l in b)
    body_phase, body_valu, body_nop, body_dep, prev_dst = collections.Counter(), 0, 0, 0, None
    for l in b:
        if re.match(r"^\s+\.loc\s", l):
            # (the comment behind a .loc names the line and every call it was inlined through; a line of a runtime header -
            #  fma(), __ballot() ... - has the phase of the line of ransac.hip that called it)
            ph = phase_of_chain([int(x) for x in LOC.findall(l.split(";", 1)[1])] if ";" in l else [])
            if ph is not None:
                cur_phase = ph
            continue
        m = re.match(r"^\s+([a-z_0-9]+)(\s|$)", l)
        if not m or l.lstrip().startswith(";") or l.lstrip().startswith("."):
            continue
        op = m.group(1)
        ph = cur_phase
        if cold and ph == "fit":
            ph = "fit_cold"
        counts[(ph, in_loop4)][opclass(op)] += 1
        if op.startswith("s_nop"):
            nop_cycles[(ph, in_loop4)] += int(l.split()[1]) + 1
        if in_loop4:
            body_phase[ph] += 1
            body_nop += op.startswith("s_nop")
            if op.startswith("v_"):
                body_valu += 1
                args = l.split(None, 1)[1].split(";")[0].split(",")
                dst = vregs(args[0])
                srcs = set().union(*[vregs(x) for x in args[1:]]) if len(args) > 1 else set()
                if op.startswith("v_fmac") or op.startswith("v_mac"):
                    srcs |= dst
                body_dep += bool(prev_dst and prev_dst & srcs)
                prev_dst = dst
            elif not (op.startswith("s_nop") or op.startswith("s_waitcnt")):
                prev_dst = None
    if in_loop4:
        bodies.append((b[0].split(":")[0], body_phase.most_common(1)[0][0], body_valu, body_nop, body_dep))

phases = ["block", "fit", "fit_cold", "score", "pre_fit", "partition", "stage1", "ring", "stage2", "single", "queue"]
classes = ["f64 arithmetic", "f32 arithmetic", "v_cvt", "v_cmp", "v_cndmask", "v_mov", "cross-lane",
           "bit ops (inlier bits, sign, bytes)", "integer / address", "other VALU", "LDS", "VMEM", "SALU", "s_nop",
           "s_waitcnt / s_barrier"]
VALU = classes[:10]


def static(p, c):
    return counts[(p, False)][c] + counts[(p, True)][c]


W = 11
print("k_ransac<64,16,6,true,true>: static instruction counts by phase and opcode class")
print("(" + (os.path.relpath(SRC, ROOT) if SRC.startswith(ROOT + os.sep) else os.path.basename(SRC) + " of --src") + (", SLP vectoriser on" if SLP else ", -fno-slp-vectorize") + "; " +
      ", ".join(f"{k} = line {v}" for k, v in sorted(L.items(), key=lambda kv: kv[1]) if k not in ("helpers_begin",)) + ")")
print()
print("class".ljust(38) + "".join(p.rjust(W) for p in phases) + "all".rjust(W))
for c in classes:
    print(c.ljust(38) + "".join(str(static(p, c)).rjust(W) for p in phases) + str(sum(static(p, c) for p in phases)).rjust(W))
print("VALU total".ljust(38) + "".join(str(sum(static(p, c) for c in VALU)).rjust(W) for p in phases) +
      str(sum(static(p, c) for c in VALU for p in phases)).rjust(W))
print("  of which in a 4-point loop body".ljust(38) + "".join(str(sum(counts[(p, True)][c] for c in VALU)).rjust(W) for p in phases))
print("s_nop idle cycles asked for".ljust(38) + "".join(str(nop_cycles[(p, False)] + nop_cycles[(p, True)]).rjust(W) for p in phases) +
      str(sum(nop_cycles.values())).rjust(W))
print("  of which in a 4-point loop body".ljust(38) + "".join(str(nop_cycles[(p, True)]).rjust(W) for p in phases))
print()
print("4-point loop bodies (dependent = VALU instructions that read the result of the VALU instruction right before them):")
for label, ph, nv, nn, nd in bodies:
    print(f"  {label.ljust(12)} {ph.ljust(8)} VALU {nv:3d}   s_nop {nn:3d}   dependent {nd:3d}")

cnt = None
if argv and os.path.exists(argv[0]):
    cnt = json.load(open(argv[0]))
if cnt:
    blocks_n = cnt["blocks_per_launch"]
    nbar = cnt["mean_block_size"]
    exact_groups = cnt["plane_fits_executed_exactly"] / 64.0
    trios = cnt["hypotheses_prescreened"] / 64.0 / 3.0
    batches = cnt["survivor_batches"]
    eligible = cnt["blocks_with_prescreen"]
    # (counts of before round 7 know no stages: every prescreened block is a single-stage one)
    single_blocks = cnt.get("widened_count_blocks_single_stage", eligible)
    two_share = (eligible - single_blocks) / max(eligible, 1.0)
    # runs per launch of each phase's straight-line part (pre_fit's static count holds the THREE unrolled fits of a
    # trio: one run per trio) ...
    runs = {"block": blocks_n, "fit": exact_groups, "fit_cold": 0.0, "score": exact_groups, "pre_fit": trios,
            "partition": eligible - single_blocks, "stage1": trios * two_share, "ring": trios * two_share,
            "stage2": cnt.get("stage_2_passes", 0.0), "single": trios * (1.0 - two_share), "queue": trios + batches}
    # ... and of its 4-point loop bodies: (point, hypothesis) pairs / 64 lanes / hypotheses per lane / 4 points
    loops = {"score": exact_groups * nbar / 4.0,
             "stage1": cnt.get("widened_count_pairs_stage_1", 0.0) / (64 * 3 * 4),
             "stage2": cnt.get("widened_count_pairs_stage_2", 0.0) / (64 * 4),
             "single": cnt.get("widened_count_pairs_single_stage", trios * 64 * 3 * nbar) / (64 * 3 * 4)}

    # the exact fit + count is inlined twice (group 0, the survivors' batches), stage 2 at every place a full ring or the
    # end of the block starts a pass: the static counts hold every copy, a run executes one of them
    copies = {p: max(1, sum(1 for b in bodies if b[1] == p)) for p in ("score", "stage2")}
    copies["fit"] = copies["score"]

    def dyn(p, table, c):
        return (table[(p, False)][c] * runs[p] + table[(p, True)][c] * loops.get(p, 0.0)) / copies.get(p, 1)

    nop_cycles_t = {k: {0: v} for k, v in nop_cycles.items()}
    for p in phases:
        for f in (False, True):
            nop_cycles_t.setdefault((p, f), {0: 0})
    print()
    print(f"dynamic estimate per launch (wave-level instructions, millions; {os.path.relpath(argv[0], ROOT)}): {blocks_n:.0f} blocks of "
          f"{nbar:.1f} points, {exact_groups / blocks_n:.2f} exact groups and {trios / blocks_n:.2f} prescreen trios per block, "
          f"{two_share:.3f} of the prescreened blocks in two stages")
    print("class".ljust(38) + "".join(p.rjust(W) for p in phases) + "total".rjust(W))
    tot_all = 0.0
    for c in classes:
        row = [dyn(p, counts, c) for p in phases]
        if c in VALU:
            tot_all += sum(row)
        print(c.ljust(38) + "".join(f"{v / 1e6:{W}.1f}" for v in row) + f"{sum(row) / 1e6:{W}.1f}")
    row = [sum(dyn(p, counts, c) for c in VALU) for p in phases]
    print("VALU total".ljust(38) + "".join(f"{v / 1e6:{W}.1f}" for v in row) + f"{tot_all / 1e6:{W}.1f}")
    row = [dyn(p, nop_cycles_t, 0) for p in phases]
    print("s_nop idle cycles asked for".ljust(38) + "".join(f"{v / 1e6:{W}.1f}" for v in row) + f"{sum(row) / 1e6:{W}.1f}")
    print("(a phase's straight-line part runs once per run of the phase - the 1-point tail loops and the 32-point outer loops "
          "included, which run up to three times / twice: an estimate, low on them - its 4-point loop bodies once per four "
          "points of the pairs the counting build counted; a phase inlined at several places runs one copy at a time: "
          + ", ".join(f"{p} / {n}" for p, n in copies.items()) + ")")
    # the counters' own total beside the estimate (a --pmc-only pass of the round)
    tag = os.path.basename(argv[0]).split("_")[0]
    sq_file, sq_keys = (SQ[0], [SQ[1]]) if SQ else (os.path.join(ROOT, "profiles", f"{tag}_sq_counters.json"), None)
    try:
        sq = json.load(open(sq_file))["kernels"]
        key = next(k for k in sq if k.startswith("k_ransac<64"))
        for who, v in sq[key].items():
            if isinstance(v, dict) and "wave_valu_instructions" in v and (sq_keys is None or who in sq_keys):
                print(f"MEASURED per launch (profiles/{os.path.basename(sq_file)}, {who}): all VALU {v['wave_valu_instructions'] / 1e6:.1f} M "
                      f"wave instructions.  Estimate / measured: {tot_all / v['wave_valu_instructions']:.2f}")
    except (OSError, KeyError, StopIteration):
        pass
