"""Per-pivot instruction mix of the four-wave twisted kernel's chain and helper loops, from the gfx950 assembly listing.

    python tools/isa_mix.py [RPL ...] [-D NAME=VALUE ...]      (default: RPL 10 12, i.e. twisted4<32,10> and <32,12>)

Compiles csrc/sls_twisted4_kernel.hip with `hipcc --cuda-device-only -S` and -DSLS_ISA_MARKS=1, which puts an assembler comment
at the start of every unrolled pivot of the chain wave's Gauss-Jordan and of the helper wave's elimination (at a sched_barrier
the code already has, so nothing moves).  The listing between two consecutive markers of the same kind is one pivot, its
out-of-line wait loop included.  A third pair of markers, "chain-tail" … "chain-tail-end", brackets what the chain wave does per
block after its last pivot (store + fused sweep step; one span per instantiated loop body, not per pivot).  Prints the registers and scratch of each instantiation and, per loop, the median count of
each instruction class per pivot.  Needs hipcc only (no GPU).
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "systemlevelcontrol.jl_amd", "csrc", "sls_twisted4_kernel.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CLASSES = [
    ("agpr copy", re.compile(r"^v_accvgpr_(read|write|mov)")),
    ("ds_swizzle", re.compile(r"^ds_swizzle")),
    ("ds_bpermute", re.compile(r"^ds_bpermute")),
    ("ds_read", re.compile(r"^ds_read")),
    ("ds_write", re.compile(r"^ds_write")),
    ("fp64", re.compile(r"^v_\w*_f64")),
    ("other valu", re.compile(r"^v_")),
    ("s_waitcnt", re.compile(r"^s_waitcnt")),
    ("branch", re.compile(r"^s_(cbranch|branch)")),
    ("other salu", re.compile(r"^s_")),
]


def compile_listing(defines):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-x", "hip", "--cuda-device-only", "-S",
           "-DSLS_ISA_MARKS=1"] + [f"-D{d}" for d in defines] + [SRC, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text


def kernel_body(text, rpl, pre=1):
    """pre = 1: the instantiation that reads the plan-time static blocks, 0: the one that rebuilds them in the launch"""
    sym = f"_ZN3sls25h2_column_twisted4_kernelILi32ELi{rpl}ELb{pre}EEEvNS_12KernelParamsE"
    beg = text.index(f"\n{sym}:")
    end = text.index(".Lfunc_end", beg)
    res = {}
    for key in ("num_vgpr", "num_agpr"):
        m = re.search(re.escape(sym) + r"\." + key + r", (\d+)", text)
        res[key] = int(m.group(1)) if m else None
    m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"(.*?)\.end_amdhsa_kernel", text, re.S)
    ms = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)) if m else None
    res["scratch"] = int(ms.group(1)) if ms else None
    return text[beg:end], res


def spans(body, mark):
    """instruction mnemonics of each span between consecutive markers `mark` (the last one ends at the next marker of any kind)"""
    out, cur = [], None
    for line in body.splitlines():
        t = line.strip()
        if t.startswith("; isa-mark"):
            if cur is not None:
                out.append(cur)
            cur = [] if t == f"; isa-mark {mark}" else None
            continue
        if cur is None or not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        cur.append(t.split()[0])
    return out


def tail_spans(body):
    """The chain wave's per-block tail, "chain-tail" … "chain-tail-end", one span per instantiated loop body.  The block placement
    may rotate the loop so that the end marker precedes the start marker in the listing: the tail then runs from the start marker
    to the first unconditional backward branch, and on from that branch's target to the end marker (side blocks placed behind the
    branch — a few instructions of divergent regions — are not counted)."""
    lines = [l.strip() for l in body.splitlines()]
    is_op = lambda t: t and not t.startswith((";", ".")) and not t.endswith(":") and ":" not in t.split()[0]
    label_at = {t.split(":")[0]: i for i, t in enumerate(lines) if t.startswith(".LBB") and ":" in t}
    out = []
    for i, t in enumerate(lines):
        if t != "; isa-mark chain-tail":
            continue
        cur, j, done = [], i + 1, False
        while j < len(lines) and not done:
            u = lines[j]
            if u == "; isa-mark chain-tail-end":
                done = True
            elif u.startswith("; isa-mark"):
                break
            elif is_op(u):
                cur.append(u.split()[0])
                tgt = u.split()[1] if u.startswith("s_branch") else None
                if tgt in label_at and label_at[tgt] < i:          # the loop's back edge: go on at its target
                    j = label_at[tgt]
            j += 1
        if done:
            out.append(cur)
    return out


def mix(mn):
    c = {name: 0 for name, _ in CLASSES}
    for op in mn:
        for name, rx in CLASSES:
            if rx.match(op):
                c[name] += 1
                break
    c["total"] = len(mn)
    return c


def main(argv):
    rpls, defines, i = [], [], 0
    while i < len(argv):
        if argv[i] == "-D":
            defines.append(argv[i + 1]); i += 2
        elif argv[i].startswith("-D"):
            defines.append(argv[i][2:]); i += 1
        else:
            rpls.append(int(argv[i])); i += 1
    text = compile_listing(defines)
    for rpl, pre in [(r, q) for r in (rpls or [10, 12]) for q in (1, 0)]:
        body, res = kernel_body(text, rpl, pre)
        print(f"twisted4<32,{rpl}> ({'plan-time blocks' if pre else 'rebuild'}): {res['num_vgpr']} VGPRs + {res['num_agpr']} AGPRs, scratch {res['scratch']} B/lane")
        for mark in ("chain-pivot", "helper-pivot", "chain-tail"):
            sp = tail_spans(body) if mark == "chain-tail" else spans(body, mark)
            if not sp:
                print(f"  {mark}: no markers found")
                continue
            ms = [mix(s) for s in sp]
            keys = ["total"] + [name for name, _ in CLASSES]
            med = {k: statistics.median(m[k] for m in ms) for k in keys}
            print(f"  {mark} ({len(sp)} {'loop bodies' if mark == 'chain-tail' else 'pivots'}), median per {'block' if mark == 'chain-tail' else 'pivot'}: " + ", ".join(f"{k} {med[k]:g}" for k in keys))
            print(f"  {mark}: agpr copies over all pivots {sum(m['agpr copy'] for m in ms)}")


if __name__ == "__main__":
    main(sys.argv[1:])
