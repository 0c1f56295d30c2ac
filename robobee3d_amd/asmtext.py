"""How a finished list of instruction tuples becomes text: the one formatter, the clobber lists, the `asm volatile` macro
block and the write-if-changed rule shared by every generator (asmgen, asmgen64, asmstep, asmqp / codegen_qp, codegen,
codegen_n3). Nothing here knows a generator: what differs between them arrives as data.

The one real difference is how integer operands are spelled. Each generator binds `fmt` to its own rule (`hex_ints`) and the
committed headers keep the bytes they have; one spelling for all is a change of its own, to be proven on code objects.
"""
import os
import re

HEX_ABOVE_64 = "above 64"       # asmstep's spelling rule: every integer operand greater than 64 prints in hex
VOP3P_KEYS = ("op_sel", "op_sel_hi", "neg_lo", "neg_hi")


def fmt(t, hex_ints=(), nt_kinds=()):
    """One instruction tuple (mnemonic, operand, ...) as one line of assembly.
    hex_ints: the mnemonics whose integer operands print in hex, or HEX_ABOVE_64.
    nt_kinds: asmqp's cache-policy rule for its global_* tuples (see below)."""
    m = t[0]
    if m == "label":
        return "%s:" % t[1]
    mods = ""
    if isinstance(t[-1], dict):          # VOP3P (packed) instruction: operands + modifiers
        d, t = t[-1], t[:-1]
        keys = ("op_sel",) if m == "v_pk_mov_b32" else VOP3P_KEYS
        mods = " " + " ".join("%s:[%s]" % (k, ",".join(map(str, d[k]))) for k in keys)
    if hex_ints == HEX_ABOVE_64:
        a = [("0x%x" % x if isinstance(x, int) and x > 64 else str(x)) for x in t[1:]]
    else:
        a = [("0x%x" % x if isinstance(x, int) and m in hex_ints else str(x)) for x in t[1:]]
    if m.startswith("ds_"):
        return "%s %s, %s offset:%s" % (m, a[0], a[1], t[3])
    if m.startswith("s_load_"):
        return "%s %s, %s, %s%s" % (m, a[0], a[1], ("0x%x" % t[3]) if isinstance(t[3], int) else t[3],
                                    (" " + t[4]) if len(t) > 4 else "")
    if m.startswith("global_") and len(t) > 4 and isinstance(t[4], int):
        # asmqp's convention (dst, off, ptr, offset[, "nt"]). Cache policy (tools/ab_qp_nt.sh): "rows" = the caller's [row][B]
        # arrays (lane offset v0: read or written once per tick), "stream" = the kernel's own per-workgroup stream blocks
        # (written once, read once, by the same workgroup); a kind listed in nt_kinds is non-temporal throughout
        kind = "rows" if (a[1] if m == "global_load_dword" else a[0]) == "v0" else "stream"
        nt = (len(a) > 4 and a[4] == "nt") or kind in nt_kinds
        return "%s %s, %s, %s offset:%s%s" % (m, a[0], a[1], a[2], a[3], " nt" if nt else "")
    if m == "s_waitcnt":
        return "s_waitcnt " + " ".join(a)
    last = t[-1] if isinstance(t[-1], str) else ""
    if m.endswith("_dpp") or last.startswith("offset:") or (m.startswith("global_") and last.startswith(("sc", "nt"))):
        return "%s %s %s" % (m, ", ".join(a[:-1]), last)      # a trailing DPP control / offset: / cache policy: no comma
    return "%s %s%s" % (m, ", ".join(a), mods)


def used_registers(ins):
    """(AGPR numbers, VGPR numbers) that appear in ANY operand of the instruction list: an over-approximation of what an
    `asm volatile` block of it may write, for exact clobber lists"""
    A, V = set(), set()
    for t in ins:
        for x in t[1:]:
            if not isinstance(x, str):
                continue
            for m_ in re.finditer(r"\b([av])\[(\d+):(\d+)\]|\b([av])(\d+)\b", x):
                if m_.group(1):
                    (A if m_.group(1) == "a" else V).update(range(int(m_.group(2)), int(m_.group(3)) + 1))
                else:
                    (A if m_.group(4) == "a" else V).add(int(m_.group(5)))
    return A, V


def clobbers(v=(), a=(), s=(), extra=()):
    """The clobber list of an `asm volatile` block that writes VGPRs v, AGPRs a and SGPRs s (register numbers); extra: entries
    spelled out by the caller. A register the block writes and this list forgets is a silent miscompile."""
    return ['"memory"', '"scc"', '"vcc"'] + list(extra) + ['"v%d"' % i for i in v] + ['"a%d"' % i for i in a] + \
           ['"s%d"' % i for i in s]


def asm_block(head, signature, ins, inputs, clob, fmt):
    """head (comment and declaration lines), then `#define <signature> asm volatile(` with one line per instruction of ins
    (pseudo-instructions already taken out by the caller, which counts what is left), the input constraints and the clobbers"""
    out = list(head) + ["#define %s asm volatile( \\" % signature]
    out += ['  "%s\\n" \\' % fmt(t) for t in ins]
    out += ["  : : %s \\" % inputs, "  : " + ", ".join(clob) + ")"]
    return "\n".join(out) + "\n"


def label_index(ins, name):
    """position of label `name` in the instruction list"""
    return ins.index(("label", name))


def write_if_changed(path, text):
    """an unchanged file is not touched: its mtime, and with it the incremental build, stay"""
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as fh:
            fh.write(text)
