"""Layer-2 MFMA control flow of the row kernels, read from the compiler's assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast --cuda-device-only -S \
        -Rpass-analysis=kernel-resource-usage rlmd_amd/csrc/rows.hip -o rows.s 2> rows_res.txt
    python tools/rows_isa.py isa rows.s [name filter ...]      # MFMA counts per kernel
    python tools/rows_isa.py res rows_res.txt [name filter ...] # the resource lines as a table
    python tools/rows_isa.py block rows.s <kernel substring> <first> <count>  # a run of MFMAs, listed

isa counts, per kernel whose mangled name holds every filter: the 16x16x32 bf16
MFMAs, those with an s_and_saveexec among the four preceding instructions (the
MFMA runs under an exec mask) and those directly followed by s_nop 7 (the
accumulator is copied before the band's next MFMA)."""
import re
import sys

MFMA = "v_mfma_f32_16x16x32_bf16"


def kernels(path):
    """{mangled name: [instruction lines]} of every function in an assembly file."""
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            name = None
            continue
        t = ln.strip()
        if not t or t.startswith((".", ";", "//")) or t.endswith(":"):
            continue
        body.append(t)
    return out


def short(name):
    m = re.search(r"(\d+)(fwd_rows_kernel|qeval_rows_kernel|cbwd_rows_kernel|abwd_rows_kernel|w2_copy_kernel)I(.*?)EEv", name)
    if not m:
        return name
    args = re.findall(r"L[ib](\d+)E", m.group(3))
    return f"{m.group(2)}<{', '.join(args)}>"


def isa(path, filt):
    print(f"{'kernel':44s} {'mfma':>5s} {'masked':>7s} {'nop7':>5s}")
    for name, body in kernels(path).items():
        if "rows_kernel" not in name or not all(f in name for f in filt):
            continue
        n = masked = nop = 0
        for i, t in enumerate(body):
            if not t.startswith(MFMA):
                continue
            n += 1
            masked += any("s_and_saveexec" in p for p in body[max(0, i - 4):i])
            nop += i + 1 < len(body) and body[i + 1].startswith("s_nop 7")
        print(f"{short(name):44s} {n:5d} {masked:7d} {nop:5d}")


def res(path, filt):
    keys = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
            "VGPRs Spill")
    print(f"{'kernel':44s} {'sgpr':>5s} {'vgpr':>5s} {'agpr':>5s} {'scratch':>8s} {'occ':>4s} {'sspill':>7s} {'vspill':>7s}")
    cur, vals = None, {}

    def flush():
        if cur and "rows_kernel" in cur and all(f in cur for f in filt):
            print(f"{short(cur):44s} " + " ".join(f"{vals.get(k, '?'):>{w}s}" for k, w in zip(keys, (5, 5, 5, 8, 4, 7, 7))))

    for ln in open(path):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            flush()
            cur, vals = m.group(1), {}
            continue
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", ln)
        if m and cur:
            vals[m.group(1)] = m.group(2)
    flush()


def block(path, sub, first, count):
    """MFMAs first .. first + count - 1 (in program order) of a kernel, from the first
    ds_read_b128 of the batch in front of them."""
    for name, body in kernels(path).items():
        if sub not in short(name).replace(" ", ""):
            continue
        at = [i for i, t in enumerate(body) if t.startswith(MFMA)]
        s, e = at[first], at[first + count - 1] + 1
        lo = at[first - 1] + 1 if first else max(0, s - 40)
        b = next((k for k in range(lo, s) if body[k].startswith("ds_read_b128")), s)
        print(f"; {short(name)}: MFMAs {first} .. {first + count - 1} of {len(at)}")
        for t in body[b:e]:
            print("\t" + t)
        return


if __name__ == "__main__":
    cmd, path, rest = sys.argv[1], sys.argv[2], sys.argv[3:]
    if cmd == "isa":
        isa(path, rest)
    elif cmd == "res":
        res(path, rest)
    else:
        block(path, rest[0], int(rest[1]), int(rest[2]))
