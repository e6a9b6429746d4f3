"""Compare the device code of two source trees kernel by kernel, without a GPU.

  python scripts/isa_diff.py OLD_CSRC NEW_CSRC

Every .hip file of both directories is compiled to gfx950 assembly with the
build's own flags (st-gcn_amd/build.py) plus
  --cuda-device-only -S -Rpass-analysis=kernel-resource-usage
and the result is cut into one record per kernel symbol, whichever file the
kernel lives in: its instruction text from the symbol's label to its end (only
the function index of the local labels .LBB<i>_<j> is normalised away, since it
counts the functions of the file) and the resource lines of the remark (VGPRs,
AGPRs, SGPRs, scratch, LDS, occupancy). Prints `same` or a unified diff per
kernel, lists the kernels only one side has, and exits non-zero on any
difference. The comparison is of text only.

OLD_CSRC is typically another commit's tree exported with git archive
(st-gcn_amd/csrc and include/, side by side as in the repository, so that the
sources' relative #include of the C header resolves). At most MAX_JOBS
compilers run at once (default 16)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-gcn_amd"))
import build  # noqa: E402

EXTRA = ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def compile_one(job):
    src, out = job
    r = subprocess.run([build.HIPCC, *build.FLAGS, *EXTRA, src, "-o", out],
                       stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"isa_diff: {src} does not compile")
    return open(out).read(), r.stderr


def kernels_of(asm, remarks):
    """{symbol: [lines]} for the kernels (.amdhsa_kernel) of one file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    text, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = text.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.strip()
        if not s or s.startswith(";"):  # blank lines, comment lines
            continue
        s = re.sub(r"\s*;.*$", "", s)  # trailing comments (instruction text has no ';')
        cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
    # remark: Function Name: <sym>, followed by one remark per resource (registers,
    # spills, scratch, LDS, occupancy): all of them belong to the record
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = res.setdefault(body.split(":", 1)[1].strip(), [])
        elif cur is not None:
            cur.append("; " + body)
    return {k: sorted(set(res.get(k, []))) + v for k, v in text.items()}


def trees(dirs, tmp, ex):
    """One {symbol: (file, record)} per directory; all files compile in one pool."""
    srcs = [sorted(f for f in os.listdir(d) if f.endswith(".hip")) for d in dirs]
    jobs = [(os.path.join(d, f), os.path.join(tmp, f"{i}_{f}.s"))
            for i, d in enumerate(dirs) for f in srcs[i]]
    done = iter(list(ex.map(compile_one, jobs)))
    out = []
    for d, files in zip(dirs, srcs):
        recs = {}
        for f in files:
            for k, v in kernels_of(*next(done)).items():
                if k in recs:
                    raise SystemExit(f"isa_diff: kernel {k} defined twice in {d}")
                recs[k] = (f, v)
        out.append(recs)
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    jobs = max(1, int(os.environ.get("MAX_JOBS", 16)))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as ex:
        old, new = trees(sys.argv[1:3], tmp, ex)
    ndiff = 0
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print(f"only in old ({old[k][0]}): {k}")
        elif k not in old:
            print(f"only in new ({new[k][0]}): {k}")
        elif old[k][1] == new[k][1]:
            where = old[k][0] if old[k][0] == new[k][0] else f"{old[k][0]} -> {new[k][0]}"
            print(f"same  {k}  [{where}, {len(new[k][1])} lines]")
            continue
        else:
            print(f"DIFF  {k}")
            sys.stdout.writelines(
                l + "\n" for l in difflib.unified_diff(old[k][1], new[k][1], old[k][0], new[k][0],
                                                       lineterm="", n=2))
        ndiff += 1
    print(f"{len(old)} kernels in old, {len(new)} in new, {ndiff} differ or are on one side only")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
