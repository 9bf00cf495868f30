"""Instruction mix of dec_upscale_kernel's prompt loop, from the device assembly of csrc/decoder_fused.hip (development).

    cd saber_amd/csrc && hipcc -O3 -std=c++17 --offload-arch=gfx950 -DSABER_OP_NS=op_bf16 -DSABER_OP_SRC='"decoder_fused.hip"' \
        --cuda-device-only -S op_wrap.hip -o /tmp/fused_bf16.s          (op_f16: -DSABER_OP_NS=op_f16 -DSABER_OP_F16=1)
    python tools/upscale_loop_count.py /tmp/fused_bf16.s

The prompt loop is the shortest backward branch that spans the kernel's MFMAs: the lines from its target label to the branch are one
iteration, one (48-token tile, prompt) unit of a wave, the rarely taken reload of the high-resolution features included.  Prints the counts per
instruction class, the plain register copies (v_mov_b32 / v_bfi_b32 with both sources equal) and the kernel's register metadata."""
import collections
import re
import sys


def main(path):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN\w+18dec_upscale_kernelE\w+:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            loops.append((i - labels[m.group(1)], labels[m.group(1)], i))
    n_mfma = sum("v_mfma" in l for l in body)
    n, a, b = min(x for x in loops if sum("v_mfma" in l for l in body[x[1]:x[2]]) == n_mfma)
    count, copies = collections.Counter(), 0
    for l in body[a:b + 1]:
        s = l.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        op = s.split()[0]
        kind = ("mfma" if op.startswith("v_mfma") else "valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else
                "vmem" if op.startswith(("buffer_", "global_", "flat_", "scratch_")) else "scalar" if op.startswith("s_") else "other")
        count[kind] += 1
        args = [x.strip() for x in s[len(op):].split(",")]
        if op == "v_mov_b32_e32" and args[1].startswith("v"):
            copies += 1
        if op == "v_bfi_b32" and args[2] == args[3]:
            copies += 1
    print(f"prompt loop: lines {start + a + 1}-{start + b + 1}: " + ", ".join(f"{k} {v}" for k, v in sorted(count.items())) + f"; register copies {copies}")
    print("metadata:", kernel_metadata(lines, "dec_upscale_kernel"))


def kernel_metadata(lines, name):
    """.vgpr_count / .vgpr_spill_count / .sgpr_spill_count of the kernel whose mangled name holds `name` (amdhsa.kernels: one '  - ' entry each)"""
    i0 = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    entry, out = [], None
    for l in lines[i0 + 1:] + ["  - "]:
        if l.startswith("  - ") or not l.startswith("  "):
            if any(re.match(r"\s+\.name:\s+\S*" + name, x) for x in entry):
                out = {m.group(1): int(m.group(2)) for x in entry for m in [re.match(r"\s+(\.vgpr_count|\.vgpr_spill_count|\.sgpr_spill_count):\s+(\d+)", x)] if m}
            entry = []
            if not l.startswith("  "):
                break
        entry.append(l)
    return out


if __name__ == "__main__":
    main(sys.argv[1])
