#!/usr/bin/env python3
"""Generates sampling_gpmpc_amd/csrc/rollout_one_gen.inc: the register-pinned leaf operations of rollout_one.hip.

rollout_one_kernel keeps a chain's whole factor in AGPRs as A operands of v_mfma_f64_4x4x4_4b_f64: a PANEL (r, g) is one FP64
register (an AGPR pair) holding tile row r of the appended labels against the four column tiles of GROUP g (unified column
tiles 4 g .. 4 g + 3, the NKT real-data tiles first; one tile per MFMA block) in the A-operand lane map: lane (kq, bm, jq)
holds L[4 r + jq][4 (4 g + bm) + kq].  Rows are appended three per step, i.e. a few LANES of a panel change per step: a VALU
instruction cannot address half of a 64-bit inline-asm operand, and a panel that hipcc is free to move gets copied around
(measured: v_accvgpr_mov / read pairs on every use).  So every panel is a C++ double that is ONLY ever touched through asm
operands with a PHYSICAL register constraint "{a[2n:2n+1]}": the register allocator then has one choice, the asm text names the
halves (a<2n>, a<2n+1>), and a masked lane update is s_mov exec + two v_accvgpr_write_b32.

Panel order (class Map; index n, registers a[2n:2n+1]): for r = 0 .. NTR-1 the groups of row r (every group in front of the
row's own tile; the own group is absent when the row's tile is the group's first block), then GD[g], g = NKT >> 2 .. : the four
diagonal tiles of group g, inverted - block b holds (L_bb^-1)^T in the natural map.  122 panels for NKT = 9, NTR = 22.

Statements: the Gram / generic chains open with s_nop 1 and close with s_nop 5 (hipcc pads nothing around inline asm); the
forward substitution of a step is ONE statement per epoch (solve_stmt) whose wait states hold the next tile row's independent
MFMAs; tools/check_dpp_hazard.py checks the ISA of the result.  The subtracting form uses the FP64 MFMA's neg modifier
(neg:[1,0,0]: -A B + C).  The append is selected by the step index (n_h = 3 t): emit_append writes the steps of every epoch and,
per (tile row, first new row), the two EXEC masks of the row's masked panel writes as constants (append_row_masks;
tests/test_one_append_masks.py checks them against the lane rule).  --steps-out FILE writes the static solve statements of
rollout_one_steps_kernel (emit_steps: one per step index) into a file of their own, which csrc/build.py generates.  --variant ... --out ...: schedule experiments of tools/ubench/one_solve_chain.hip.
"""
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sampling_gpmpc_amd", "csrc", "rollout_one_gen.inc")
MF = "v_mfma_f64_4x4x4_4b_f64"


VARIANT = set()   # schedule experiments of tools/ubench/one_solve_chain.hip (--variant a,b,...); the shipped file has none
NKT = 9           # real-data column tiles (N_r = 36)
NTR = 22          # tile rows of appended labels (3 (H - 1) <= 88)


def u_of(r):
    return NKT + r


class Map:
    """panel (r, g): tile row r of the appended labels against column GROUP g (unified column tiles 4 g .. 4 g + 3, the
    real-data tiles first); the group that holds the row's own diagonal tile stops in front of it and is absent when the
    diagonal tile is the group's first block."""
    def __init__(self):
        self.idx = {}
        self.groups = {}
        n = 0
        for r in range(NTR):
            u = u_of(r)
            gs = list(range(u >> 2)) + ([u >> 2] if (u & 3) else [])
            self.groups[r] = gs
            for g in gs:
                self.idx[("p", r, g)] = n; n += 1
        self.gd = list(range(NKT >> 2, (u_of(NTR - 1) >> 2) + 1))
        for g in self.gd:
            self.idx[("gd", g, 0)] = n; n += 1
        self.count = n
        assert 2 * n <= 256, "panels exceed the AGPR file"

    def reg(self, kind, a, b):
        return 2 * self.idx[(kind, a, b)]


def chain_stmt(items, neg, fresh=False):
    """items: list of (areg or None, a_expr, b_expr): one asm statement accumulating alternately into c0 / c1.
    areg None: the A operand is an ordinary VGPR value.  fresh: the accumulators start at zero (SrcC = 0 in the first MFMA of
    each: no v_mov of zeros in front of every chain); needs at least two MFMAs."""
    head, tail, acc_first = True, "s_nop 5", 0
    lines = ['"s_nop 1\\n\\t"']
    ops_in = []
    k = len(items)
    assert not fresh or k >= 2
    for i, (areg, aexpr, bexpr) in enumerate(items):
        c = (i + acc_first) & 1
        a_txt = f"a[{areg}:{areg + 1}]" if areg is not None else f"%{2 + 2 * i}"
        b_txt = f"%{2 + 2 * i + 1}"
        src_c = "0" if (fresh and i < 2) else f"%{c}"
        lines.append(f'"{MF} %{c}, {a_txt}, {b_txt}, {src_c}{" neg:[1,0,0]" if neg else ""}\\n\\t"')
        if i + 1 < k:
            lines.append('"s_nop 1\\n\\t"')
        ops_in.append(f'"{{a[{areg}:{areg + 1}]}}"({aexpr})' if areg is not None else f'"v"({aexpr})')
        ops_in.append(f'"v"({bexpr})')
    if tail:
        lines.append(f'"{tail}"')
    else:
        lines[-1] = lines[-1][:-5] + '"'          # drop the trailing \n\t of the last instruction
    body = "\n        ".join(lines)
    cons = '"=&v"(c0), "=&v"(c1)' if fresh else '"+v"(c0), "+v"(c1)'
    return f"    asm volatile({body}\n        : {cons}\n        : {', '.join(ops_in)});\n"



# ---- the forward substitution of one step as ONE statement ------------------------------------------------------------------
# Registers of the statement (the kernel itself stays below v214; build.py / the ISA check assert it):
#   v[216 + 2 g : 217 + 2 g]   Vu[g], the solution of column group g (tied operands with a physical constraint: the DPP merge
#                              writes HALVES of it under a bank mask, and inline asm cannot name half of a %operand)
#   v[232:233] T   v[234:235] T2 (the rotated copy)   v[236:237] W   v[238:245] X0 .. X3: the accumulators of two tile rows
#   v[246:247] RNm: the row's right-hand side masked to the row's own block (the start value of its second accumulator)
#   v[248:249], v[250:251] G0 / G1: the accumulators of the Gram product S' = sum_g Vu[g]^T Vu[g] (outputs of the statement)
SOLVE_VU, SOLVE_T, SOLVE_T2, SOLVE_W, SOLVE_X, SOLVE_RNM, SOLVE_G = 216, 232, 234, 236, 238, 246, 248
SOLVE_CLOBBER = list(range(232, 248))


# The inverse of group K's diagonal tiles rides in the statement of every epoch K >= SOLVE_INV_KMIN (group 2's rows are the
# statement's first rows: nothing stands in front of them to hide it behind).
SOLVE_INV_KMIN = 3


def vp(n):
    return f"v[{n}:{n + 1}]"


def inverse_ops(m, K):
    """The diagonal tiles of group K, inverted inside one_solve<K>: U^-1 = (I + M)(I + M^2) D^-1 with U = D (I - M) - the
    operations, operands and order of rollout_one.hip's inverse_tiles (the same bits), as the stages solve_stmt places in the
    wait states of tile rows 0 and 1.  Temporaries: RNm's register (a clobber of the statement) and the two Gram accumulators
    (early-clobber outputs, free until the step's last tile row).  %[ud] / %[dr] / %[dc] / %[inat]: the kernel's loop-carried
    L^T of the lane's tile, 1 / diag along its rows / columns, the identity in the natural map."""
    X, Y, Z = SOLVE_RNM, SOLVE_G, SOLVE_G + 2
    n = m.reg("gd", K, 0)
    return {"m": [f"v_fma_f64 {vp(X)}, -%[dr], %[ud], %[inat]"],                       # M = I - drow ud
            "f1": [f"{MF} {vp(Y)}, {vp(X)}, %[inat], 0"],                             # M^T
            "f2": [f"{MF} {vp(Z)}, {vp(Y)}, {vp(X)}, 0"],                              # M M
            "add": [f"v_add_f64 {vp(Y)}, %[inat], {vp(Y)}", f"v_add_f64 {vp(Z)}, %[inat], {vp(Z)}"],
            "f3": [f"{MF} {vp(X)}, {vp(Y)}, {vp(Z)}, 0"],                              # (I + M)(I + M^2)
            "put": [f"v_mul_f64 {vp(X)}, %[dc], {vp(X)}",
                    f"v_accvgpr_write_b32 a{n}, v{X}", f"v_accvgpr_write_b32 a{n + 1}, v{X + 1}"]}


def solve_stmt(f, m, K, member, nh=None):
    """Row r: acc = rhs_r - sum_g panel(r, g) Vu[g]; W = G_r (block sum of acc); block b of Vu[g_r] := W.  Left to the compiler
    (one statement per chain, per MFMA, per DPP pair) every MFMA result is fenced by s_nop 5 (the compiler neither sees the
    MFMA nor may it schedule into the statement), twice per row: 48 of a row's ~190 cycles.  Here the row is software
    pipelined by hand: only the row's LAST panel (the group that holds tile r - 1) depends on the previous row, the others are
    issued INSIDE the previous row - behind its dependent MFMA, behind its diagonal MFMA and in the wait states in front of
    the three DPP reads (tools/ubench/mfma64_fill.hip: ONE independent FP64 MFMA between an MFMA and the reader of its result
    leaves nothing to pad).  The rows that may be absent this step (4 r >= n_h) are left by scalar branches inside the
    statement; the last row of a step has nothing to hide behind and takes the padded form.

    nh: the STATIC form for a step that finds exactly nh rows (one_solve_t<t>, nh = 3 t in epoch K): only the rows with 4 r < nh,
    the last of them in the nxt = None form reached by fall-through, no compare, branch, label or nh operand - the MFMA, DPP and
    VALU instructions of the run-time statement's path for that nh, in its order, with its operands; only the padding differs."""
    R0 = 4 * K - NKT
    STATIC = nh is not None
    assert not STATIC or (K == epoch_of(nh // T_ROWS) and nh % T_ROWS == 0)
    rows = list(range(0, min(R0 + 4, NTR)))
    if STATIC:
        rows = [r for r in rows if 4 * r < nh]
    L = []
    used = []

    def areg(kind, x, y):
        n = m.reg(kind, x, y)
        used.append((n, member(x, y) if kind == "p" else f"P.gd[{x}]"))
        return f"a[{n}:{n + 1}]"
    VU = lambda g: SOLVE_VU + 2 * g
    T, T2, W = SOLVE_T, SOLVE_T2, SOLVE_W
    accs = lambda r: (SOLVE_X + 4 * (r & 1), SOLVE_X + 4 * (r & 1) + 2)
    INV = K >= SOLVE_INV_KMIN and "noinv" not in VARIANT
    inv = inverse_ops(m, K) if INV else {}
    NOUT = K + 1 + 2 + (1 if INV else 0)                # Vu[0 .. K], S0, S1, (gd[K])
    rn_op = lambda g: f"%{NOUT + (g - m.gd[0])}"
    nh_op = f"%{NOUT + (K - m.gd[0] + 1)}"
    mk_op = lambda b: f"%{NOUT + (K - m.gd[0] + 1) + (0 if STATIC else 1) + b}"      # 1.0 in the lanes of block b, 0.0 elsewhere
    GRAM = "nogram" not in VARIANT

    def gram_items(gs):
        """S' += Vu[g]^T Vu[g] (a natural register used as the A operand acts as its transpose): the step's Gram product rides in
        the wait states of the LAST tile row - which has no next row to hide behind - and behind its merge"""
        return [("gram", f"{MF} {vp(SOLVE_G + 2 * (g & 1))}, {vp(VU(g))}, {vp(VU(g))}, {'0' if g < 2 else vp(SOLVE_G + 2 * (g & 1))}")
                for g in gs]
    RNM = SOLVE_RNM
    # --variant rnfold: the right-hand side starts the row's second accumulator (masked to the row's block) instead of being
    # added on the chain.  Measured (tools/ubench/one_solve_chain.hip, 22 rows): -3 cycles per row alone, +6 together with the
    # post-merge MFMA below - not shipped.
    FOLD = "rnfold" in VARIANT
    assert not (FOLD and INV), "RNm's register holds the inverse's M"

    def ra_list(r):
        # (accumulator, A panel, B register, start value: None = accumulate)
        return [(accs(r)[i & 1], areg("p", r, g), VU(g), (vp(RNM) if (i == 1 and FOLD) else "0") if i < 2 else None)
                for i, g in enumerate(m.groups[r][:-1])]

    def emit_ra(item):
        if item[0] == "gram":
            L.append(item[1])
            return
        acc, a, b, start = item
        L.append(f"{MF} {vp(acc)}, {a}, {vp(b)}, {start if start is not None else vp(acc)} neg:[1,0,0]")

    def emit_rnm(r):
        """RNm of row r: rhs_r in the lanes of the row's own block only - the cross-block sum then adds it exactly once, and the
        `+ rhs` add leaves the row's dependent chain (one FP64 multiply by a 0 / 1 mask, off the chain)"""
        u = u_of(r)
        L.append(f"v_mul_f64 {vp(RNM)}, {rn_op(u >> 2)}, {mk_op(u & 3)}")

    def rot(ctrl):
        L.append(f"v_mov_b32_dpp v{T2}, v{T} {ctrl} row_mask:0xf bank_mask:0xf bound_ctrl:1")
        L.append(f"v_mov_b32_dpp v{T2 + 1}, v{T + 1} {ctrl} row_mask:0xf bank_mask:0xf bound_ctrl:1")
        L.append(f"v_add_f64 {vp(T)}, {vp(T)}, {vp(T2)}")

    def row(r, nxt, head=True):
        """nxt: the independent MFMAs of row r + 1 (None: the step's last row - the Gram products of the groups in front of
        the row's own stand in their place, the own group's follows the merge); head: the statement in front ended on the merge
        (VALU write of Vu[dep] -> MFMA read: two wait states).  Returns whether the NEXT row needs that head."""
        u = u_of(r)
        g, b = u >> 2, u & 3
        last = nxt is None
        if last and GRAM:
            nxt = gram_items(range(0, g))
        c0, c1 = accs(r)
        dep = m.groups[r][-1]
        n_ind = len(m.groups[r]) - 1
        dacc = accs(r)[n_ind & 1]                       # the accumulator the independent MFMAs did not write last
        q = list(nxt) if nxt is not None else []
        # one MFMA of the next row is kept for BEHIND the merge, where the next row's dependent MFMA would wait for Vu[dep]
        post = q.pop() if (len(q) >= 3 and "nopost" not in VARIANT) else None
        keep = 1                                        # (one stays for behind the diagonal MFMA)

        # The inverse of group K's tiles, spread over the wait states of rows 0 and 1 (always present for K >= 3, their slots
        # are s_nop otherwise: the next row has two independent MFMAs).  Distances (tools/check_dpp_hazard.py, the strict
        # count): M -> f1 4 states, f1 -> f2 9, f2 -> the adds 8, the adds -> f3 3, f3 -> the product 8; the pair of writes
        # stands a whole tile row in front of the first MFMA that reads gd[K] (row 4 K - NKT >= 3).
        stage = {}
        if INV and r == 0:
            stage = {1: inv["m"], 2: inv["f1"], "c": inv["f2"]}
        elif INV and r == 1:
            stage = {1: inv["add"], 2: inv["f3"], "c": inv["put"]}
        assert not stage or (not last and len(q) <= 2)
        nslot = [0]

        def slot(pad):
            """an MFMA of the next row where a wait would stand (it counts as one state for a VALU -> DPP / MFMA read)"""
            nslot[0] += 1
            if nslot[0] in stage:                       # a stage of the inverse: every instruction is one state
                L.extend(stage[nslot[0]])
                if len(stage[nslot[0]]) <= pad:
                    L.append(f"s_nop {pad - len(stage[nslot[0]])}")
            elif len(q) > keep and "noslots" not in VARIANT:
                emit_ra(q.pop(0))
                L.append("s_nop 0")
            else:
                L.append(f"s_nop {pad}")
        if not last and FOLD:
            emit_rnm(r + 1)                             # (read by the next row's second MFMA, in a slot below)
            if head:
                L.append("s_nop 0")
        elif head:
            L.append("s_nop 1")                         # the merge in front wrote Vu[dep]: VALU write -> MFMA read
        L.append(f"{MF} {vp(dacc)}, {areg('p', r, dep)}, {vp(VU(dep))}, {vp(dacc)} neg:[1,0,0]")
        if q:
            emit_ra(q.pop(0))
        else:
            L.append("s_nop 5")
        L.append(f"v_add_f64 {vp(T)}, {vp(c0)}, {vp(c1)}")
        if "nosum" in VARIANT:                          # (timing floor only: wrong results)
            L.append(f"v_add_f64 {vp(T)}, {vp(T)}, {rn_op(g)}")
            slot(1)
        else:
            slot(1)
            rot("row_ror:8")
            slot(1)
            rot("row_ror:4")
            if not FOLD:
                L.append(f"v_add_f64 {vp(T)}, {vp(T)}, {rn_op(g)}")
            slot(1)
        L.append(f"{MF} {vp(W)}, {areg('gd', g, 0)}, {vp(T)}, 0")
        if q:
            while q:
                emit_ra(q.pop(0))
                if q and "nomfmanop" not in VARIANT:
                    L.append("s_nop 1")
            if "c" in stage:                            # behind an independent MFMA: nothing is left to pad for the merge
                if stage["c"][0].startswith(MF):
                    L.append("s_nop 1")
                L.extend(stage["c"])
        elif "c" in stage:
            L.extend(stage["c"])
            if not stage["c"][0].startswith(MF):
                L.append(f"s_nop {5 - len(stage['c'])}")
        else:
            L.append("s_nop 5")
        L.append(f"v_mov_b32_dpp v{VU(g)}, v{W} quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0x{1 << b:x}")
        L.append(f"v_mov_b32_dpp v{VU(g) + 1}, v{W + 1} quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0x{1 << b:x}")
        if post is not None:
            emit_ra(post)
            L.append("s_nop 0")
            if not last:
                return False
        if last and GRAM:                               # the own group's Gram product: Vu[g] was merged two instructions ago
            if post is None:
                L.append("s_nop 1")
            emit_ra(gram_items([g])[0])
        return True

    def gram_only():
        """no appended row yet: the Gram product of the real-data tiles alone"""
        if GRAM:
            L.append("s_nop 1")
            for i, it in enumerate(gram_items(range(0, K + 1))):
                if i:
                    L.append("s_nop 1")
                emit_ra(it)

    def prologue():
        if FOLD:
            emit_rnm(0)
        L.append("s_nop 1")
        first = ra_list(0)
        for i, it in enumerate(first):
            emit_ra(it)
            if i + 1 < len(first):
                L.append("s_nop 1")

    if STATIC:
        if rows:
            prologue()
            head = False
            for r in rows:
                head = row(r, ra_list(r + 1) if r + 1 in rows else None, head)
        else:
            gram_only()
    else:
        if R0 <= 0:
            L.append(f"s_cmp_eq_u32 {nh_op}, 0")
            L.append("s_cbranch_scc1 .Lone_none_%=")
        prologue()
        lasts = []
        head = False                                        # (the prologue ends on MFMAs)
        for r in rows:
            if r + 1 in rows:
                if r + 1 >= R0:                             # row r + 1 may be absent this step
                    L.append(f"s_cmp_gt_u32 {nh_op}, {4 * (r + 1)}")
                    L.append(f"s_cbranch_scc0 .Lone_last{r}_%=")
                    lasts.append((r, head))
                head = row(r, ra_list(r + 1), head)
            else:
                row(r, None, head)
        L.append("s_branch .Lone_end_%=")
        for r, hd in lasts:
            L.append(f".Lone_last{r}_%=:")
            row(r, None, True)                              # (reached by a branch: padded whatever stood in front - 8 cycles per step)
            L.append("s_branch .Lone_end_%=")
        if R0 <= 0:
            L.append(".Lone_none_%=:")
            gram_only()
        else:
            L.pop()                                         # the last of them falls through
        L.append(".Lone_end_%=:")
    if GRAM:
        L.append("s_nop 5")                             # S0 / S1 are read by the compiler's code next
    seen, ins = set(), []
    if INV:
        seen.add(m.reg("gd", K, 0))                     # written here: an output
    for n, mem in used:
        if n not in seen:
            seen.add(n)
            ins.append(f'"{{a[{n}:{n + 1}]}}"({mem})')
    outs = ", ".join(f'"+{{v[{VU(g)}:{VU(g) + 1}]}}"(Vu[{g}])' for g in range(K + 1))
    outs += f', "=&{{v[{SOLVE_G}:{SOLVE_G + 1}]}}"(S0), "=&{{v[{SOLVE_G + 2}:{SOLVE_G + 3}]}}"(S1)'
    if INV:
        n = m.reg("gd", K, 0)
        outs += f', "+{{a[{n}:{n + 1}]}}"(P.gd[{K}])'
    rn = ", ".join(f'"v"(RN[{g}])' for g in range(m.gd[0], K + 1))
    mk = ", ".join(f'"v"(MK[{b}])' for b in range(4))
    if INV:
        mk += ', [ud] "v"(ud), [dr] "v"(drow), [dc] "v"(dcol), [inat] "v"(inat)'
    clob = ", ".join(f'"v{n}"' for n in SOLVE_CLOBBER) + ', "scc"'
    body = "\n        ".join(f'"{x}\\n\\t"' for x in L[:-1]) + f'\n        "{L[-1]}"'
    if STATIC:
        clob = ", ".join(f'"v{n}"' for n in SOLVE_CLOBBER)
        # (the block masks are read by the rnfold variant only: as operands of the shipped statement they would pin eight
        # registers for nothing - the static steps have none to spare in the last two epochs)
        mk = ", ".join(([f'"v"(MK[{b}])' for b in range(4)] if FOLD else []) +
                       (['[ud] "v"(ud), [dr] "v"(drow), [dc] "v"(dcol), [inat] "v"(inat)'] if INV else []))
        ins_txt = ", ".join(x for x in (mk, ("\n          " + ", ".join(ins)) if ins else "") if x)
        ins_txt = ", " + ins_txt if ins_txt else ""
        f.write(f"__device__ __forceinline__ void one_solve_t_{nh // T_ROWS}(OnePanels& P, double* Vu, const double* RN, const double* MK, double& S0, double& S1, double ud, double drow, double dcol, double inat) {{\n")
        f.write(f"    asm volatile({body}\n        : {outs}\n        : {rn}{ins_txt}\n        : {clob});\n}}\n")
        return
    f.write(f"__device__ __forceinline__ void one_solve_{K}(OnePanels& P, double* Vu, const double* RN, const double* MK, int nh, double& S0, double& S1, double ud, double drow, double dcol, double inat) {{\n")
    f.write(f"    asm volatile({body}\n        : {outs}\n        : {rn}, \"s\"(nh), {mk},\n          {', '.join(ins)}\n        : {clob});\n}}\n")


def set_stmt(items, mask="mask"):
    """items: list of (areg, member_expr, value_expr): masked lane update of up to 6 panels in one statement."""
    k = len(items)
    # operands: 0 = saved exec, 1.. = k tied panels, then mask, then lo / hi pairs
    # an empty mask skips the writes INSIDE the statement: a C++ `if` around a tied physical-register operand makes hipcc keep
    # the panel in a virtual register across the branch (copies in and out of the pinned register, spills of the rest)
    lines = ['"s_mov_b64 %0, exec\\n\\t"', f'"s_mov_b64 exec, %{1 + k}\\n\\t"', '"s_cbranch_execz .Lone_skip_%=\\n\\t"']
    outs = ['"=&s"(sv_)']
    ins = [f'"s"({mask})']
    for i, (areg, member, val) in enumerate(items):
        outs.append(f'"+{{a[{areg}:{areg + 1}]}}"({member})')
        lo = 2 + k + 2 * i
        lines.append(f'"v_accvgpr_write_b32 a{areg}, %{lo}\\n\\t"')
        lines.append(f'"v_accvgpr_write_b32 a{areg + 1}, %{lo + 1}\\n\\t"')
        ins.append(f'"v"(__double2loint({val}))')
        ins.append(f'"v"(__double2hiint({val}))')
    lines.append('".Lone_skip_%=:\\n\\t"')
    lines.append('"s_mov_b64 exec, %0"')
    body = "\n        ".join(lines)
    return f"    asm volatile({body}\n        : {', '.join(outs)}\n        : {', '.join(ins)});\n"


def hidden_set_stmt(items, mask):
    """the same masked update WITHOUT naming the panels as operands: for use under a C++ branch (a tied physical-register
    operand defined inside a branch makes hipcc carry the panel in a virtual register across it); one_touch() afterwards tells
    the compiler that the panels may have changed.  EXEC IS ALL ONES where these stand (the kernel is launched 64 lanes wide
    and the step's control flow is uniform): nothing is saved, EXEC is restored to -1."""
    k = len(items)
    lines = ['"s_mov_b64 exec, %0\\n\\t"']
    ins = [f'"s"({mask})']
    for i, (areg, val) in enumerate(items):
        lo = 1 + 2 * i
        lines.append(f'"v_accvgpr_write_b32 a{areg}, %{lo}\\n\\t"')
        lines.append(f'"v_accvgpr_write_b32 a{areg + 1}, %{lo + 1}\\n\\t"')
        ins.append(f'"v"(__double2loint({val}))')
        ins.append(f'"v"(__double2hiint({val}))')
    lines.append('"s_mov_b64 exec, -1"')
    body = "\n        ".join(lines)
    return f"    asm volatile({body}\n        :\n        : {', '.join(ins)});\n"


def put_stmt(items):
    """items: list of (areg, member_expr, value_expr): every lane of up to 6 panels - no EXEC handling at all (EXEC is all ones)"""
    lines, outs, ins = [], [], []
    k = len(items)
    for i, (areg, member, val) in enumerate(items):
        outs.append(f'"+{{a[{areg}:{areg + 1}]}}"({member})')
        lo = k + 2 * i
        lines.append(f'"v_accvgpr_write_b32 a{areg}, %{lo}\\n\\t"')
        lines.append(f'"v_accvgpr_write_b32 a{areg + 1}, %{lo + 1}\\n\\t"')
        ins.append(f'"v"(__double2loint({val}))')
        ins.append(f'"v"(__double2hiint({val}))')
    lines[-1] = lines[-1][:-5] + '"'
    body = "\n        ".join(lines)
    return f"    asm volatile({body}\n        : {', '.join(outs)}\n        : {', '.join(ins)});\n"


# ---- the append of a step as code selection: n_h = 3 t is static ----------------------------------------------------------------
# rollout_one_kernel runs unseeded launches only and every step but the last appends T = 3 rows, so step t finds n_h = 3 t rows
# and everything its append selects by - the incomplete tile row, the lanes of the new rows, the EXEC masks of the panel writes
# - is a function of t alone.  The kernel dispatches on t once per step (one_pick_row over the epoch's steps) and the masks
# below reach the masked writes as 64-bit constants.
T_ROWS = 3
APPEND_STEPS = (4 * NTR) // T_ROWS            # steps t = 0 .. 28 append (rows 3 t .. 3 t + 2 of the 88)


def epoch_of(t):
    """group K of the incomplete tile when step t starts (the step loop's epoch)"""
    return (NKT + ((T_ROWS * t) >> 2)) >> 2


def epoch_steps(K):
    """the steps t of epoch K as range(begin, end), from the loop condition ((NKT + (n_h >> 2)) >> 2) == K with n_h = 3 t"""
    lo4, hi4 = 4 * (4 * K - NKT), 4 * (4 * K + 4 - NKT)          # n_h in [lo4, hi4)
    begin = max(0, -(-lo4 // T_ROWS))
    end = min(max(begin, -(-hi4 // T_ROWS)), APPEND_STEPS + 1)   # (H <= 30: the last step, t = 29, appends nothing)
    return range(begin, end)


def append_rows(t):
    """the tile rows that receive lanes in step t: the incomplete one and, when the three new rows reach into it, the next"""
    nh = T_ROWS * t
    tn = nh >> 2
    return [tn] + ([tn + 1] if (nh & 3) >= 2 and tn + 1 < NTR else [])


def append_row_masks(r, nh):
    """(mBase, mLast) of one_hset_row_<r> when rows nh .. nh + 2 are appended: lane (kq, bm, jq) = 16 kq + 4 bm + jq holds row
    4 r + jq of the panel; mBase = the lanes of the new rows (the full groups), mLast = those of the blocks in front of the
    row's own diagonal tile (block (NKT + r) & 3 of its group).  Zero when no new row lies in tile row r."""
    j0, j1 = max(nh - 4 * r, 0), min(nh + T_ROWS - 4 * r, 4)
    nib = sum(1 << j for j in range(j0, j1))                     # the new rows' jq inside one block
    b = u_of(r) & 3
    row16 = sum(nib << (4 * bm) for bm in range(b))              # the blocks bm < b of one DPP row (one kq)
    return nib * 0x1111111111111111, row16 * 0x0001000100010001


# ---- the lanes of the 3 x 3 root of (S + noise): the static steps run ONE root stream -----------------------------------------
# The factor C = chol(S + noise) and 1 / diag(C) are read by the append's selects alone (rollout_one.hip: OnePatReach,
# OnePatDiag, OnePatInvRow, OnePatInvCol for the step's group and, when rows wrap, for the next one), each lane-locally: the lanes
# that receive one of these values are a function of t.  In them the root stream factors S + noise, in all others S - the root the
# draw needs, whose slots 1 and 2 are consumed in the lane of the step's point alone.
KPT0 = 4 + 9                                  # appended point j lives in lane KPT0 + j (behind the N0 + N1 axis lanes)
KLAST = (NKT + NTR - 1) >> 2                  # the last group that holds diagonal tiles


def _new_entry_is_root(ri, rk):
    """one_new_entry: True where the entry of new row ri against column rk (same origin) is a value of C"""
    return 0 <= rk <= ri


def root_patterns(t):
    """{pattern name: lanes that receive a value of C or 1 / diag(C)} for the selects step t's block applies"""
    nh = T_ROWS * t
    i0, tn, K = nh & 3, nh >> 2, epoch_of(t)
    bt, lo = (NKT + tn) & 3, nh - 4 * (4 * K - NKT)
    out = {}
    if t >= APPEND_STEPS:
        return out

    def lanes(pred):
        return sum(1 << l for l in range(64) if pred(l >> 4, (l >> 2) & 3, l & 3))

    def group(tag, LO):
        out["diag" + tag] = lanes(lambda kq, bm, jq: 0 <= 4 * bm + jq - LO < T_ROWS and _new_entry_is_root(4 * bm + jq - LO, 4 * bm + kq - LO))
        out["invrow" + tag] = lanes(lambda kq, bm, jq: 0 <= 4 * bm + kq - LO < T_ROWS)
        out["invcol" + tag] = lanes(lambda kq, bm, jq: 0 <= 4 * bm + jq - LO < T_ROWS)

    if i0 >= 2 and tn + 1 < NTR:
        out["reach"] = lanes(lambda kq, bm, jq: bm == bt and jq < i0 - 1 and kq >= i0 and _new_entry_is_root(4 + jq - i0, kq - i0))
    group("", lo)
    if K < KLAST and lo + T_ROWS > 16:
        group("1", lo - 16)
    return out


def root_lanes(t):
    """A_t: the lanes in which step t's root stream factors S + noise"""
    m = 0
    for v in root_patterns(t).values():
        m |= v
    return m


def root_draw_lane(t):
    """r_t: the lane the draw's slots 1 and 2 are taken from - the lane of the step's point when it factors S, the highest
    lane that does otherwise"""
    a = root_lanes(t)
    if not (a >> (KPT0 + t)) & 1:
        return KPT0 + t
    return max(l for l in range(64) if not (a >> l) & 1)


def emit_root_lanes(f):
    f.write("// ---- the root stream of static step t: lanes that factor S + noise (every other lane factors S), the draw's lane ---------\n")
    f.write("template <int TS> struct OneRootLanes;\n")
    for t in range(APPEND_STEPS + 1):
        f.write(f"template <> struct OneRootLanes<{t}> {{ static constexpr unsigned long long value = 0x{root_lanes(t):016x}ull; "
                f"static constexpr int draw = {root_draw_lane(t)}; }};\n")


def emit_append(f):
    f.write("// ---- the append of step t, n_h = 3 t: the steps of an epoch and the EXEC masks of the panel writes as constants ------------\n")
    f.write(f"constexpr int kOneAppendSteps = {APPEND_STEPS};\n")
    f.write("template <int K> struct OneEpoch;\n")
    for K in Map().gd:
        s = epoch_steps(K)
        f.write(f"template <> struct OneEpoch<{K}> {{ static constexpr int t_begin = {s.start}, t_end = {s.stop}; }};\n")
    f.write("template <int R, int NH> struct OneRowMask;\n")
    for t in range(APPEND_STEPS):
        for r in append_rows(t):
            mb, ml = append_row_masks(r, T_ROWS * t)
            f.write(f"template <> struct OneRowMask<{r}, {T_ROWS * t}> {{ static constexpr unsigned long long base = 0x{mb:016x}ull, last = 0x{ml:016x}ull; }};\n")
    f.write("// the masked writes of tile row R for the new rows NH .. NH + 2 (hidden form: see one_hset_row)\n")
    f.write("template <int R, int NH>\n__device__ __forceinline__ void one_hset_row_at(const double* V) {\n"
            "    one_hset_row<R>(OneRowMask<R, NH>::base, OneRowMask<R, NH>::last, V);\n}\n")


def emit(f):
    m = Map()
    f.write(f"// ---- NKT = {NKT}, {NTR} tile rows: {m.count} panels in a[0:{2 * m.count - 1}] ----------------------------------------------------\n")
    f.write(f"struct OnePanels {{\n    double p[{m.count - len(m.gd)}];\n    double gd[{max(m.gd) + 1}];\n}};\n")
    f.write(f"constexpr int kOneNKT = {NKT}, kOneNTR = {NTR};\n")
    f.write(f"constexpr int kOneSolveInvK = {SOLVE_INV_KMIN};      // one_solve<K> inverts group K's diagonal tiles for K >= this\n")
    member = lambda r, g: f"P.p[{m.idx[('p', r, g)]}]"
    for r in range(NTR):
        gs = m.groups[r]
        # off-diagonal part of tile row r: c -= panel(r, g) Vu[g]  (block b of the product: column tile 4 g + b)
        f.write(f"__device__ __forceinline__ void one_row_{r}(OnePanels& P, double& c0, double& c1, const double* Vu) {{\n")
        f.write(chain_stmt([(m.reg("p", r, g), member(r, g), f"Vu[{g}]") for g in gs], True, fresh=True))
        f.write("}\n")
        # masked lane update: the full groups under mBase, the row's own (partial) group under mLast
        u = u_of(r)
        full = [g for g in gs if g < (u >> 2)]
        f.write(f"__device__ __forceinline__ void one_set_row_{r}(OnePanels& P, unsigned long long mBase, unsigned long long mLast, const double* V) {{\n    unsigned long long sv_;\n    (void)mLast;\n")
        for s in range(0, len(full), 6):
            f.write(set_stmt([(m.reg("p", r, g), member(r, g), f"V[{g}]") for g in full[s:s + 6]], "mBase"))
        if u & 3:
            g = u >> 2
            f.write(set_stmt([(m.reg("p", r, g), member(r, g), f"V[{g}]")], "mLast"))
        f.write("}\n")
    for r in range(NTR):
        u = u_of(r)
        full = [g for g in m.groups[r] if g < (u >> 2)]
        f.write(f"__device__ __forceinline__ void one_hset_row_{r}(unsigned long long mBase, unsigned long long mLast, const double* V) {{\n    (void)mLast;\n")
        for s_ in range(0, len(full), 12):
            f.write(hidden_set_stmt([(m.reg("p", r, g), f"V[{g}]") for g in full[s_:s_ + 12]], "mBase"))
        if u & 3:
            g = u >> 2
            f.write(hidden_set_stmt([(m.reg("p", r, g), f"V[{g}]")], "mLast"))
        f.write("}\n")
    # "the panels of tile rows R .. R + N - 1 may have changed": empty statements with tied operands
    f.write("template <int R>\n__device__ __forceinline__ void one_touch_row(OnePanels& P) {\n")
    for r in range(NTR):
        ops = ", ".join([f'"+{{a[{m.reg("p", r, g)}:{m.reg("p", r, g) + 1}]}}"({member(r, g)})' for g in m.groups[r]])
        f.write(f"    {'if' if r == 0 else 'else if'} constexpr (R == {r}) asm volatile(\"\" : {ops});\n")
    f.write("}\n")
    for g in m.gd:
        a = m.reg("gd", g, 0)
        f.write(f"__device__ __forceinline__ double one_gdm_{g}(OnePanels& P, double acc) {{\n    double d;\n"
                f"    asm volatile(\"s_nop 1\\n\\t{MF} %0, a[{a}:{a + 1}], %2, 0\\n\\ts_nop 5\" : \"=&v\"(d) : \"{{a[{a}:{a + 1}]}}\"(P.gd[{g}]), \"v\"(acc));\n"
                f"    return d;\n}}\n")
        f.write(f"__device__ __forceinline__ void one_hset_gd_{g}(double v) {{\n"
                f"    asm volatile(\"v_accvgpr_write_b32 a{a}, %0\\n\\tv_accvgpr_write_b32 a{a + 1}, %1\" : : \"v\"(__double2loint(v)), \"v\"(__double2hiint(v)));\n}}\n")
        f.write(f"__device__ __forceinline__ void one_touch_gd_{g}(OnePanels& P) {{ asm volatile(\"\" : \"+{{a[{a}:{a + 1}]}}\"(P.gd[{g}])); }}\n")
        f.write(f"__device__ __forceinline__ void one_put_gd_{g}(OnePanels& P, double v) {{\n")
        f.write(put_stmt([(a, f"P.gd[{g}]", "v")]))
        f.write("}\n")
    # everything to zero, the diagonal tiles to the identity
    f.write("__device__ __forceinline__ void one_init(OnePanels& P, double inat) {\n    double z = 0.0;\n")
    allp = [(m.reg("p", r, g), member(r, g), "z") for r in range(NTR) for g in m.groups[r]]
    for s in range(0, len(allp), 6):
        f.write(put_stmt(allp[s:s + 6]))
    for g in m.gd:
        f.write(put_stmt([(m.reg("gd", g, 0), f"P.gd[{g}]", "inat")]))
    f.write("}\n")

    def disp(name, ret, params, args, rng):
        f.write(f"template <int R>\n__device__ __forceinline__ {ret} {name}({params}) {{\n")
        for i, r in enumerate(rng):
            f.write(f"    {'if' if i == 0 else 'else if'} constexpr (R == {r}) {'return ' if ret != 'void' else ''}{name}_{r}({args});\n")
        f.write("}\n")
    disp("one_row", "void", "OnePanels& P, double& c0, double& c1, const double* Vu", "P, c0, c1, Vu", range(NTR))
    disp("one_set_row", "void", "OnePanels& P, unsigned long long mBase, unsigned long long mLast, const double* V", "P, mBase, mLast, V", range(NTR))
    for K in m.gd:
        solve_stmt(f, m, K, member)
    disp("one_solve", "void", "OnePanels& P, double* Vu, const double* RN, const double* MK, int nh, double& S0, double& S1, double ud, double drow, double dcol, double inat", "P, Vu, RN, MK, nh, S0, S1, ud, drow, dcol, inat", m.gd)
    disp("one_hset_row", "void", "unsigned long long mBase, unsigned long long mLast, const double* V", "mBase, mLast, V", range(NTR))
    disp("one_gdm", "double", "OnePanels& P, double acc", "P, acc", m.gd)
    disp("one_put_gd", "void", "OnePanels& P, double v", "P, v", m.gd)
    disp("one_hset_gd", "void", "double v", "v", m.gd)
    disp("one_touch_gd", "void", "OnePanels& P", "P", m.gd)
    emit_append(f)
    emit_root_lanes(f)


def emit_steps(f):
    """rollout_one_steps_gen.inc: the static solve statements one_solve_t<t>, one per step index t with n_h = 3 t
    (rollout_one_steps_kernel).  7 400 lines that repeat what the run-time statements hold, so the file is NOT committed:
    csrc/build.py writes it (--steps-out) before it compiles, tests/test_one_steps_stmt.py checks the statements it holds."""
    m = Map()
    member = lambda r, g: f"P.p[{m.idx[('p', r, g)]}]"
    steps = range(APPEND_STEPS + 1)
    for t in steps:
        solve_stmt(f, m, epoch_of(t), member, nh=T_ROWS * t)
    sig = "OnePanels& P, double* Vu, const double* RN, const double* MK, double& S0, double& S1, double ud, double drow, double dcol, double inat"
    f.write(f"template <int R>\n__device__ __forceinline__ void one_solve_t({sig}) {{\n")
    for t in steps:
        f.write(f"    {'if' if t == 0 else 'else if'} constexpr (R == {t}) one_solve_t_{t}(P, Vu, RN, MK, S0, S1, ud, drow, dcol, inat);\n")
    f.write("}\n")


def generic(f):
    """chains with every operand in ordinary registers (the LDS-resident super row, the Gram products)"""
    for neg, fresh in ((False, False), (True, False), (False, True)):
        nm = "one_fchain" if fresh else ("one_nchain" if neg else "one_pchain")
        for k in range(2 if fresh else 1, 13):
            args = ", ".join([f"double a{i}" for i in range(k)] + [f"double b{i}" for i in range(k)])
            items = [(None, f"a{i}", f"b{i}") for i in range(k)]
            f.write(f"__device__ __forceinline__ void {nm}{k}(double& c0, double& c1, {args}) {{\n")
            f.write(chain_stmt(items, neg, fresh))
            f.write("}\n")
        f.write(f"template <int K>\n__device__ __forceinline__ void {nm}(double& c0, double& c1, const double* A, const double* B) {{\n")
        for k in range(2 if fresh else 1, 13):
            call = ", ".join([f"A[{i}]" for i in range(k)] + [f"B[{i}]" for i in range(k)])
            f.write(f"    {'if' if k == (2 if fresh else 1) else 'else if'} constexpr (K == {k}) {nm}{k}(c0, c1, {call});\n")
        f.write("}\n")


if __name__ == "__main__":
    if "--variant" in sys.argv:
        VARIANT = set(sys.argv[sys.argv.index("--variant") + 1].split(","))
    if "--steps-out" in sys.argv:                   # the static statements alone, into their own (uncommitted) file
        path = sys.argv[sys.argv.index("--steps-out") + 1]
        with open(path, "w") as f:
            f.write("// GENERATED by tools/gen_rollout_one.py --steps-out - do not edit, do not commit.  The static solve statements of rollout_one.hip.\n")
            emit_steps(f)
        print(path)
        sys.exit(0)
    if "--out" in sys.argv:
        OUT = sys.argv[sys.argv.index("--out") + 1]
    with open(OUT, "w") as f:
        f.write("// GENERATED by tools/gen_rollout_one.py - do not edit.  Register-pinned panel operations of rollout_one.hip.\n")
        generic(f)
        emit(f)
    print(OUT)
