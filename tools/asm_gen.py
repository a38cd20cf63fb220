"""What the three generators of the gfx950 traversal loops share (gen_skip_asm.py, gen_skip2_asm.py, gen_flat_asm.py): the line collector
and its rendering as an inline-assembly string, VGPR pairs and the packed-math emitters with their op_sel encoding, the three-bank rotation
of the hierarchy walks, the clobber-list wrapper, the header writer -- and the table of scalar registers the loops use WITHOUT declaring
them, with the `; rt-loops` marker tools/check_reserved_registers.py finds those statements by.

The lean f32 square root has exactly ONE copy, here: its arithmetic has to equal sqrt_rn_lean (rt_math.hpp), the sequence rt_selftest_sqrt
holds against the IEEE root on all 2^32 inputs on the device.  Three hand-kept copies were three chances to drift from what that test
checks; what the loops really differ in (their registers, how "a needed lane is tiny" is decided, which mask holds the zero test) is the
RootRegs record.

Not a program: the generators import it, each after making its own directory importable."""
import collections
import re


class Asm:
    def __init__(self):
        self.lines = []

    def op(self, text, comment=None):
        self.lines.append(("\t", text, comment))

    def label(self, name):
        self.lines.append(("", name + ":", None))

    def extend(self, other):
        self.lines.extend(other.lines)

    def render(self, indent="        "):
        out = []
        for tab, text, comment in self.lines:
            s = '%s"%s%s\\n"' % (indent, "" if tab == "" else "\\t", text)
            if comment:
                s += "  /* %s */" % comment
            out.append(s)
        return "\n".join(out)


class Pair:
    """A VGPR pair: .p the pair, .h[0] / .h[1] its halves (ray 0 / ray 1)."""

    def __init__(self, lo):
        self.p = "v[%d:%d]" % (lo, lo + 1)
        self.h = ("v%d" % lo, "v%d" % (lo + 1))


def sp(first, n=2):
    return "s[%d:%d]" % (first, first + n - 1)


# ------------------------------------------------------------------------------------------------------------- packed math

def _packed(a, mnemonic, dst, srcs, scalars, neg_y, comment):
    """A scalar operand is either half of an ALIGNED SGPR pair, broadcast to both results: op_sel / op_sel_hi pick the half."""
    srcs, sel, sel_hi = list(srcs), [0] * len(srcs), [1] * len(srcs)
    for i, s in enumerate(scalars):
        if s is not None:
            srcs[i] = sp(s & ~1)
            sel[i] = sel_hi[i] = s & 1
    mods = ""
    if any(sel):
        mods += " op_sel:[%s]" % ",".join("%d" % b for b in sel)
    if not all(sel_hi):
        mods += " op_sel_hi:[%s]" % ",".join("%d" % b for b in sel_hi)
    if neg_y:
        mods += " neg_lo:[0,1] neg_hi:[0,1]"
    a.op("%s %s, %s%s" % (mnemonic, dst, ", ".join(srcs), mods), comment)


def pk(a, op, dst, x, y, sx=None, sy=None, neg_y=False, comment=None):
    """dst = x op y on both rays.  sx / sy: SGPR NUMBER whose value is broadcast to both rays in place of a VGPR pair."""
    _packed(a, "v_pk_%s_f32" % op, dst, (x, y), (sx, sy), neg_y, comment)


def pk_fma(a, dst, x, y, z, sx=None, sy=None, sz=None, comment=None):
    """dst = x * y + z on both rays, ONE rounding (the conservative filters only; never on the exact path).  sx / sy / sz as in pk."""
    _packed(a, "v_pk_fma_f32", dst, (x, y, z), (sx, sy, sz), False, comment)


# ------------------------------------------------------------------------------------------------------- the lean f32 root

# t0, t1: scratch; scaled: the tiny path's operand; root: the result; tiny: SGPR pair of the lanes below 2^-96; zero: the mask of the tiny
# path's +-0 test ("vcc": the VOP2 encodings); need: the SGPR pair `tiny & need_mask` is formed in -- None where every lane of EXEC is
# needed (the flat scan narrows EXEC to the candidates), and then any tiny lane takes the scaled path.
RootRegs = collections.namedtuple("RootRegs", "t0 t1 scaled root tiny zero need")


def refine(a, R, x):
    """R.t0 = y ~ 1/sqrt(x) (v_rsq_f32, 1 ulp)  ->  R.root = the correctly rounded sqrt(x): g = x*y, h = y/2, r = x - g*g (exact,
    one FMA), root = g + r*h (one FMA).  Equal to the IEEE root for every finite x >= 2^-96 (checked on the device against
    all of them: rt_selftest_sqrt runs the same sequence, sqrt_rn_lean in rt_math.hpp)."""
    a.op("v_mul_f32_e32 %s, %s, %s" % (R.root, x, R.t0), "g = x*y")
    a.op("v_mul_f32_e32 %s, 0.5, %s" % (R.t0, R.t0), "h = y/2")
    a.op("v_fma_f32 %s, -%s, %s, %s" % (R.t1, R.root, R.root, x), "r = x - g*g")
    a.op("v_fma_f32 %s, %s, %s, %s" % (R.root, R.t1, R.t0, R.root), "g + r*h")


def root(a, R, x, need_mask, done_label, tiny_label):
    """Correctly rounded sqrt(x) into R.root (== sqrt_rn_lean).  need_mask: the lanes whose root is used (R.need None: those in EXEC)."""
    a.op("v_rsq_f32_e32 %s, %s" % (R.t0, x))
    a.op("v_cmp_lt_f32_e64 %s, |%s|, %%[tiny]" % (R.tiny, x))
    if R.need is None:
        a.op("s_cmp_lg_u64 %s, 0" % R.tiny)
        a.op("s_cbranch_scc1 %s" % tiny_label, "a lane below 2^-96 (zero included): scaled path")
    else:
        a.op("s_and_b64 %s, %s, %s" % (R.need, R.tiny, need_mask))
        a.op("s_cbranch_scc1 %s" % tiny_label, "some needed lane below 2^-96 (zero included): scaled path")
    refine(a, R, x)
    a.label(done_label)


def tiny(a, R, x, tiny_label, done_label):
    """The cold half of root(): the same two FMAs on x * 2^64 in the lanes of R.tiny, the result scaled back by 2^-32."""
    a.label(tiny_label)
    a.op("v_mul_f32_e32 %s, 0x5f800000, %s" % (R.t0, x), "root with the 2^64 / 2^-32 scaling for tiny lanes (the scaled operand stays >= 2^-85: its residual is never subnormal)")
    a.op("v_cndmask_b32_e64 %s, %s, %s, %s" % (R.scaled, x, R.t0, R.tiny))
    a.op("v_rsq_f32_e32 %s, %s" % (R.t0, R.scaled))
    enc = "e32" if R.zero == "vcc" else "e64"
    a.op("v_cmp_eq_f32_%s %s, 0, %s" % (enc, R.zero, R.scaled), "sqrt(+-0) = +-0 (rsq would make it 0 * inf)")
    refine(a, R, R.scaled)
    a.op("v_cndmask_b32_%s %s, %s, %s, %s" % (enc, R.root, R.root, R.scaled, R.zero))
    a.op("v_mul_f32_e32 %s, 0x2f800000, %s" % (R.t0, R.root))
    a.op("v_cndmask_b32_e64 %s, %s, %s, %s" % (R.root, R.root, R.t0, R.tiny))
    a.op("s_branch %s" % done_label)


# ------------------------------------------------------------------------------------------------- the three-bank rotation

class Rotation:
    """The hierarchy walks' three copies of the loop body over three scalar register banks (gen_skip_asm.py documents the walk): a step ends
    in the copy whose current-node bank already holds the successor it chose.  prefix: of every label; nx: the register that holds the
    offset behind the current node; stride: a node's size in bytes."""
    COPIES = {"A": (0, 1, 2), "B": (1, 0, 2), "C": (2, 0, 1)}      # current, next, skip
    NEXT_COPY = {"A": "B", "B": "A", "C": "A"}
    SKIP_COPY = {"A": "C", "B": "C", "C": "B"}
    LAYOUT = "ACB"                                                 # main paths in this order: A.skip and C.skip fall through
    FLAG_LIMIT = "0x3fffffff"                                      # item word above this: ITEM (bit 31) or END (bit 30)

    def __init__(self, prefix, nx, stride):
        self.prefix, self.nx, self.stride = prefix, nx, stride

    def lab(self, name):
        """The labels of copy `name`, as a function of their short name."""
        return lambda x: "%s%s_%s_%%=" % (self.prefix, name, x)

    def top_of(self, name):
        return "%s%s_top_%%=" % (self.prefix, name)

    def emit_skip(self, a, name, skip_reg):
        """`skip` transition: the successor is the node behind the subtree (an ITEM's own successor)."""
        a.label(self.lab(name)("skip"))
        a.op("s_add_u32 %s, %s, %d" % (self.nx, skip_reg, self.stride), "jump over the subtree")
        a.op("s_waitcnt lgkmcnt(0)")
        nxt = self.SKIP_COPY[name]
        if self.LAYOUT.index(nxt) != self.LAYOUT.index(name) + 1:  # A -> C and C -> B fall through
            a.op("s_branch %s" % self.top_of(nxt))

    def emit_next(self, a, name):
        a.op("s_add_u32 %s, %s, %d" % (self.nx, self.nx, self.stride))
        a.op("s_waitcnt lgkmcnt(0)")
        a.op("s_branch %s" % self.top_of(self.NEXT_COPY[name]))

    def assemble(self, a, copy_fn):
        """copy_fn(name) -> (main path, cold paths) of one copy: the main paths in LAYOUT order, the cold ones behind them."""
        parts = {name: copy_fn(name) for name in "ABC"}
        for name in self.LAYOUT:
            a.extend(parts[name][0])
        for name in "ABC":
            a.extend(parts[name][1])


# ------------------------------------------------------------------------------------------------------ statements, files

def clobber_list(sgprs, vgprs=()):
    """The clobber list of a statement that owns these scalar / vector register numbers, wrapped like the rest of the header."""
    regs = ['"s%d"' % r for r in sgprs] + ['"v%d"' % r for r in vgprs]
    lines, cur = [], '"memory", "vcc", "scc"'
    for r in regs:
        if len(cur) + len(r) + 2 > 118:
            lines.append(cur + ",")
            cur = "          " + r
        else:
            cur += ", " + r
    lines.append(cur)
    return "\n".join(lines)


def write_header(out, text):
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out, "(%d lines)" % text.count("\n"))


# Registers the compiler RESERVES in the one kernel a flavour's loops are built into are not named in their clobber lists: it never allocates
# them, so there is nothing to tell it -- and naming them is what `-Winline-asm` ("clobber list contains reserved registers") objects to.
# That the loops may use them rests on the kernel's .sgpr_count (the hardware's allocation covers them) and on no compiler-generated
# instruction touching them: tests/test_kernel_resources.py checks both on the generated assembly (tools/check_reserved_registers.py).
# Flavour -> (name prefixes of the kernels its loops are written for, the registers):
#   two-ray   s32: the stack pointer of a kernel that has no stack (reserved in every kernel); s[72:73] under amdgpu_waves_per_eu(8)
#   f64       k_render_skip_f64: amdgpu_num_sgpr(96) + amdgpu_waves_per_eu(7) leave the compiler s[0:87]
#   f64-lo    the low-window copies of the f64 loops (s[20:73]): s32 again
UNDECLARED = {"two-ray": (("void rt::k_render_skip2<", "void rt::k_render_skip2_fast<"), (32, 72, 73)),
              "f64": (("void rt::k_render_skip_f64<", "void rt::k_render_skip_f64_coop<"), (88, 89)),
              "f64-lo": (("void rt::k_render_skip_fast64_coop<",), (32,))}


def loops_marker(flavour):
    """The comment a statement that leaves registers undeclared starts with; it survives into the compiler's assembly output."""
    regs = UNDECLARED[flavour][1]
    runs = [[regs[0], regs[0]]]
    for r in regs[1:]:
        if r == runs[-1][1] + 1:
            runs[-1][1] = r
        else:
            runs.append([r, r])
    # (the spelling of the committed headers: a lone register among several runs is s32, a whole set is always a range)
    return "; rt-loops %s: undeclared %s" % (flavour, ", ".join("s%d" % lo if lo == hi and len(runs) > 1 else sp(lo, hi - lo + 1) for lo, hi in runs))


def marker_flavour(line):
    """The flavour whose marker an assembly line carries, or None."""
    m = re.search(r"; rt-loops ([\w-]+): undeclared", line)
    return m.group(1) if m else None
