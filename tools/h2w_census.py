"""Static instruction census of conv3d_k3_h2w_kernel's march (csrc/kernels/conv3d_wino_h2.h) from hipcc's assembly, one row per template form.
Development aid; needs no GPU:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Imonai_amd/csrc --cuda-device-only -S <tu>.hip -o h2w.s
    python tools/h2w_census.py h2w.s [label]
where <tu>.hip includes kernels/conv3d_wino_h2.h and instantiates the forms (capi.hip itself works too).  A "loop" is the span between a label and the LAST backward
branch to it; the march loops are the spans with at least 36 matrix instructions that contain no other such span.  The counts are static: every arm of a branch inside
the span is included.  The kernel's register count, scratch size and spill count come from the metadata at the end of the file."""
import re
import sys

FORMS = {"ILb1ELb0ELb0E": "plain + stats <1,0,0>", "ILb1ELb1ELb0E": "accumulating <1,1,0>", "ILb1ELb0ELb1E": "pooling <1,0,1>", "ILb0ELb0ELb0E": "plain <0,0,0>"}
COLS = ["mfma", "vector", "packed", "v_mov_b32", "v_mov_b64", "select", "v_add_u32", "v_readfirstlane", "scalar", "s_and_saveexec", "branch", "s_nop", "s_waitcnt", "barrier", "lds", "vmem"]


def classify(op):
    """-> the census columns one instruction counts in"""
    if op.startswith("v_mfma"):
        return ["mfma"]
    if op.startswith(("ds_",)):
        return ["lds"]
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return ["vmem"]
    if op.startswith("v_"):
        c = ["vector"]
        if op.startswith("v_pk_"):
            c.append("packed")
        if op.startswith("v_mov_b32"):
            c.append("v_mov_b32")
        if op.startswith("v_mov_b64"):
            c.append("v_mov_b64")
        if op.startswith("v_cndmask"):
            c.append("select")
        if op.startswith("v_add_u32"):
            c.append("v_add_u32")
        if op.startswith("v_readfirstlane"):
            c.append("v_readfirstlane")
        return c
    if op.startswith(("s_cbranch", "s_branch")):
        return ["branch"]
    if op.startswith("s_nop"):
        return ["s_nop"]
    if op.startswith("s_waitcnt"):
        return ["s_waitcnt"]
    if op.startswith("s_barrier"):
        return ["barrier"]
    if op.startswith("s_"):
        return ["scalar"] + (["s_and_saveexec"] if op.startswith("s_and_saveexec") else [])
    return []


def kernels(lines):
    """-> {mangled name: (first line, last line)} of the h2w kernels' bodies"""
    out, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2mh20conv3d_k3_h2w_kernel\w+):", l)
        if m:
            cur = (m.group(1), i)
        elif cur and l.strip().startswith("s_endpgm"):
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def loops(lines, lo, hi):
    labels = {}
    spans = {}
    for i in range(lo, hi):
        l = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
            continue
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels:
            spans[labels[m.group(1)]] = i       # the last backward branch to that label
    return sorted(spans.items())


def census(lines, a, b):
    c = dict.fromkeys(COLS, 0)
    for i in range(a, b + 1):
        m = re.match(r"^\s+([a-z_0-9]+)", lines[i])
        if not m:
            continue
        for k in classify(m.group(1)):
            c[k] += 1
    return c


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    with open(path) as f:
        text = f.read()
    lines = text.split("\n")
    print(f"== {label}")
    for name, (lo, hi) in kernels(lines).items():
        form = next((v for k, v in FORMS.items() if k in name), name)
        meta = text[text.index(".name:           " + name):]
        regs = {k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1)) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
        print(f"-- {form}: vgpr {regs['vgpr_count']} sgpr {regs['sgpr_count']} spills {regs['vgpr_spill_count']} scratch {regs['private_segment_fixed_size']} bytes; "
              f"kernel {hi - lo} lines")
        big = [(a, b) for a, b in loops(lines, lo, hi) if census(lines, a, b)["mfma"] >= 36]
        inner = [(a, b) for a, b in big if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in big)]
        for a, b in inner:
            c = census(lines, a, b)
            planes = c["mfma"] // 36
            print(f"   loop lines {a - lo}..{b - lo} ({planes} planes): " + " ".join(f"{k}={c[k]}" for k in COLS))
            print("      per plane: " + " ".join(f"{k}={c[k] / planes:.1f}" for k in ("vector", "scalar", "branch", "lds", "vmem")))


if __name__ == "__main__":
    main()
