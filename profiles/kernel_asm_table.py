"""Per-kernel table of the gfx950 code of every .hip file of a csrc directory, and the comparison of two such tables: the
check that a change which moves or re-dispatches kernels leaves every kernel's instructions and resources as they were.

  python profiles/kernel_asm_table.py table CSRC_DIR OUT.tsv      device code of every CSRC_DIR/*.hip with the flags of
                                                                  krylovfspssa_amd/build.py plus --offload-device-only -S
  python profiles/kernel_asm_table.py compare A.tsv B.tsv OUT.tsv one row per kernel symbol of either side, and the verdict

A kernel is what stands between its label and its .amdhsa_kernel block.  Its body is hashed with comments dropped and the
numbers of local labels (.LBB<n>_<m>, .Lfunc_end<n>: n counts the functions of the file in order of instantiation) taken
out; the descriptor block (.amdhsa_* lines: registers, LDS, scratch, kernel arguments) is hashed as it stands.  Runs on
any machine with hipcc: no device is needed."""
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I/opt/rocm/include", "-Wno-ignored-attributes",
         "--offload-device-only", "-S"]
COLUMNS = ["symbol", "file", "body", "lines", "vgpr", "sgpr", "lds", "scratch", "descriptor"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def kernels_of(asm):
    """{symbol: (body hash, body lines, vgpr, sgpr, lds, scratch, descriptor hash)} of one assembly file"""
    lines = asm.split("\n")
    label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^([A-Za-z_][\w$.]*):", l)) and not l.startswith(".L")}
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        desc = [x.strip() for x in lines[i + 1:end]]
        body = []
        for x in lines[label[sym] + 1:i]:
            x = re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0]).strip()
            if x and not x.startswith((".section", ".p2align")):
                body.append(re.sub(r"\s+", " ", x))
        val = {d.split()[0]: d.split()[1] for d in desc if len(d.split()) == 2}
        out[sym] = (hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body), val[".amdhsa_next_free_vgpr"],
                    val[".amdhsa_next_free_sgpr"], val[".amdhsa_group_segment_fixed_size"], val[".amdhsa_private_segment_fixed_size"],
                    hashlib.sha256("\n".join(desc).encode()).hexdigest()[:16])
    return out


def _compile(src, tmp):
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    subprocess.run([_hipcc()] + FLAGS + [src, "-o", out], check=True, stderr=subprocess.DEVNULL, cwd=os.path.dirname(src))
    return os.path.basename(src), kernels_of(open(out).read())


def table(csrc, path):
    srcs = sorted(glob.glob(os.path.join(os.path.abspath(csrc), "*.hip")))
    rows = []
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as pool:
        for name, ks in pool.map(lambda s: _compile(s, tmp), srcs):
            rows += [(sym, name) + k for sym, k in ks.items()]
    rows.sort()
    with open(path, "w") as f:
        f.write("\t".join(COLUMNS) + "\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    print(f"{len(rows)} kernels of {len(srcs)} files -> {path}")


def _read(path):
    by = {}
    for l in open(path).read().split("\n")[1:]:
        if l:
            r = l.split("\t")
            by.setdefault(r[0], []).append(r[1:])
    return by


def compare(pa, pb, path):
    a, b = _read(pa), _read(pb)
    both = sorted(set(a) & set(b))
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    # a library's template kernels (rocprim) are emitted by every file that uses them, as weak copies, on both sides alike:
    # what counts is a symbol with more copies than it had
    twice = [s for s in both if len(b[s]) > len(a[s])] + [s for s in only_b if len(b[s]) > 1]
    differ = [s for s in both if sorted(r[1:] for r in a[s]) != sorted(r[1:] for r in b[s])]
    moved = [s for s in both if sorted(r[0] for r in a[s]) != sorted(r[0] for r in b[s])]
    verdict = (f"{len(a)} symbols in the first table, {len(b)} in the second; only in the first {len(only_a)}, only in the second "
               f"{len(only_b)}, emitted in more files than before {len(twice)}, body or descriptor differs {len(differ)}, "
               f"in another file {len(moved)}")
    ok = not (only_a or only_b or twice or differ)
    with open(path, "w") as f:
        f.write(f"# {verdict}: {'IDENTICAL' if ok else 'DIFFERENT'}\n")
        f.write("# rows: the project's own kernels (namespace kfsp), one file each; the counts above cover every symbol\n")
        f.write("\t".join(["symbol", "file_a", "file_b", "equal", "body_a", "body_b", "lines", "vgpr", "sgpr", "lds", "scratch",
                           "descriptor_a", "descriptor_b"]) + "\n")
        for s in sorted(set(a) | set(b)):
            if not s.startswith("_ZN4kfsp"):
                continue
            ra, rb = a.get(s, [["-"] * 8])[0], b.get(s, [["-"] * 8])[0]
            f.write("\t".join([s, ra[0], rb[0], "yes" if ra[1:] == rb[1:] else "NO", ra[1], rb[1]] + rb[2:7] + [ra[7], rb[7]]) + "\n")
    print(verdict)
    for s in (only_a + only_b + twice + differ)[:40]:
        print("  ", s[:200])
    print("IDENTICAL" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "table":
        table(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4]))
    else:
        sys.exit(__doc__)
