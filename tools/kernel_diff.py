#!/usr/bin/env python3
"""Compare the gfx950 device code of the convolution objects of two builds, kernel by kernel.

    python tools/kernel_diff.py OBJ_DIR_A OBJ_DIR_B [--prefix conv_igemm]

For every PREFIX*.o of a directory (obj-gan_amd/csrc/build of a tree) the gfx950 code object is pulled out of the fat
binary and disassembled; kernels are keyed by mangled symbol over ALL objects of the directory, so a kernel may move
between files.  A kernel's text is normalised before hashing: `//` comments (they carry absolute addresses), blank
and `...` lines, and the s_nop / s_code_end padding behind the last s_endpgm are dropped.  Prints the symbol-set
difference and the kernels whose text differs; exit status 1 on any.  The check for "host-only" changes.
"""
import glob, hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels(obj_dir, prefix):
    """{mangled kernel symbol: sha1 of its normalised disassembly} over obj_dir/prefix*.o"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(obj_dir, prefix + "*.o"))):
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
            run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
            if os.path.getsize(fat) == 0:       # host-only object: no device code
                continue
            run("clang-offload-bundler", "--type=o", "--unbundle", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
            # kernels are the functions with a kernel descriptor SYM.kd next to them
            names = set(re.findall(r"\s(\S+)\.kd$", run("llvm-readelf", "-s", "-W", co), re.M))
            text = run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co)
        sym, body = None, []

        def flush():
            if sym in names:
                while body and body[-1].split()[0] in ("s_nop", "s_code_end"):
                    body.pop()
                assert sym not in out, "kernel %s defined twice" % sym
                out[sym] = hashlib.sha1("\n".join(body).encode()).hexdigest()
        for line in text.splitlines():
            m = re.match(r"^<(\S+)>:$", line.strip())
            if m:
                flush()
                sym, body = m.group(1), []
                continue
            line = line.split("//")[0].strip()
            if line and line != "...":
                body.append(line)
        flush()
    return out


def main(argv):
    prefix = "conv_igemm"
    if "--prefix" in argv:
        i = argv.index("--prefix")
        prefix = argv[i + 1]
        del argv[i:i + 2]
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(argv[1], prefix), kernels(argv[2], prefix)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("kernels: %d in A, %d in B; only in A: %d, only in B: %d, text differs: %d"
          % (len(a), len(b), len(only_a), len(only_b), len(differ)))
    for tag, names in (("only in A", only_a), ("only in B", only_b), ("differs", differ)):
        for k in names:
            print("  %s: %s" % (tag, k))
    return 1 if (only_a or only_b or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
