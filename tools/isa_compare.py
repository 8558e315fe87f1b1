"""Compare the gfx950 machine code of the register-tree kernels with another revision's, on the CPU:

    python tools/isa_compare.py REV  [> profiles/tree_isa_compare.txt]

sc_kernel.hip, scq_kernel.hip, scf_kernel.hip, ae_kernel.hip and genie_kernel.hip are compiled to assembly
twice, from `git show REV:` copies of csrc/ and the C header in a temporary directory and from the working
tree, as build() compiles them (tests/test_scq_resources.py).  Per kernel of REV: the register counts, spills,
private and LDS bytes of the metadata, the instruction counts by class and the mnemonic-sequence hash
(tests/test_kernel_resources.py isa_summary).  Exit status 1 unless both trees have the same kernels with equal
metadata and equal class counts; a kernel whose hash alone differs is marked "reordered".
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "polar-code-pytorch-sionna_amd"), os.path.join(ROOT, "tests")]
import test_kernel_resources as t  # noqa: E402
from polar_amd import build  # noqa: E402

FILES = ["sc_kernel.hip", "scq_kernel.hip", "scf_kernel.hip", "ae_kernel.hip", "genie_kernel.hip"]
CSRC_REL = os.path.relpath(build.CSRC, ROOT)
HEADER_REL = os.path.relpath(build.HEADER, ROOT)
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size")
CLASSES = ("valu", "salu", "vmem", "lds", "smem", "dpp", "total")


def checkout(rev, td):
    """csrc/ and the C header of `rev`, at their paths relative to the repository, under td."""
    names = subprocess.run(["git", "ls-tree", "-r", "-z", "--name-only", rev, CSRC_REL, HEADER_REL], cwd=ROOT,
                           check=True, capture_output=True, text=True).stdout.split("\0")
    for name in filter(None, names):
        path = os.path.join(td, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(subprocess.run(["git", "show", f"{rev}:{name}"], cwd=ROOT, check=True, capture_output=True).stdout)
    return os.path.join(td, CSRC_REL)


def assembly(csrc, td):
    """{file: gfx950 assembly} of FILES under csrc, with build.COMPILE_FLAGS minus -fPIC."""
    def one(name):
        out = os.path.join(td, name + ".s")
        cmd = [t.HIPCC, f"--offload-arch={build.ARCH}", *[f for f in build.COMPILE_FLAGS if f != "-fPIC"],
               "--cuda-device-only", "-S", os.path.join(csrc, name), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr[-4000:])
        return open(out).read()
    with ThreadPoolExecutor(max_workers=len(FILES)) as ex:
        return dict(zip(FILES, ex.map(one, FILES)))


def summary(asm):
    """{kernel: metadata fields and isa_summary} of one assembly file."""
    meta = t._kernel_meta(asm, lambda n: True)
    for block in asm.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name]["agpr_count"] = int(re.match(r":\s+(\d+)", block).group(1))
        meta[name]["sgpr_count"] = int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1))
    isa = t.isa_summary(asm, lambda n: n in meta)
    return {k: {**meta[k], **isa[k]} for k in meta}


def compare(old, new, out=sys.stdout):
    """Prints one line per kernel of `old` = {file: assembly}; returns the number of failures."""
    bad = 0
    print("kernel  " + " ".join(k.replace("_count", "").replace("_segment_fixed_size", "") for k in META) + " | " +
          " ".join(CLASSES) + " sha | verdict", file=out)
    for name in FILES:
        a, b = summary(old[name]), summary(new[name])
        print(f"# {name}: {len(a)} kernels", file=out)
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                bad += 1
                print(f"{k}  only in the {'old' if k in a else 'new'} tree: FAIL", file=out)
                continue
            diff = [f"{f} {a[k][f]} -> {b[k][f]}" for f in META + CLASSES if a[k][f] != b[k][f]]
            verdict = "FAIL: " + ", ".join(diff) if diff else "same" if a[k]["sha"] == b[k]["sha"] else \
                f"reordered (sha {b[k]['sha']})"
            bad += bool(diff)
            print(f"{k}  " + " ".join(str(a[k][f]) for f in META) + " | " + " ".join(str(a[k][f]) for f in CLASSES) +
                  f" {a[k]['sha']} | {verdict}", file=out)
    return bad


def main(rev):
    with tempfile.TemporaryDirectory() as td:
        old_dir, new_dir = os.path.join(td, "old"), os.path.join(td, "new")
        os.makedirs(new_dir)
        old = assembly(checkout(rev, old_dir), old_dir)
        new = assembly(build.CSRC, new_dir)

    def git(*args):
        return subprocess.run(["git", *args], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    print(f"# register-tree kernels: {git('rev-parse', '--short', rev).strip()} against the working tree")
    # a kernel of a file whose sources did not change compares equal to itself: evidence of nothing
    changed = [os.path.basename(f) for f in git("diff", "--name-only", rev, "--", CSRC_REL, HEADER_REL).split()]
    print("# sources that differ: " + (", ".join(changed) or "none"))
    bad = compare(old, new)
    print(f"# {bad} kernels differ in metadata or class counts")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
