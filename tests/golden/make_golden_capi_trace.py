"""Builds and runs tests/capi_trace.hip (the host-path trace of csrc/qpal_capi.hip; no GPU, no torch) and records
tests/golden/capi_trace.txt.

    python tests/golden/make_golden_capi_trace.py [--capi PATH] [--check]

--capi PATH  trace this qpal_capi.hip instead of the tree's (an earlier commit's, say: `git show REV:q-palette_amd/csrc/qpal_capi.hip`)
--check      compare with the golden file instead of writing it; exit status 1 and the differing cases on a mismatch

The golden file is a record of what the host path computed BEFORE a change: a refactor of qpal_capi.hip must leave it alone, and a
change of the planner's decisions re-records it on purpose.  tests/test_capi_and_host.py uses the helpers below.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "q-palette_amd", "csrc")
GOLDEN = os.path.join(HERE, "capi_trace.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# one child process per setting (the library reads its knobs once): the full sweep with no knob set, a reduced one under the
# knobs bench.py and the tests use
RUNS = [
    ("default", {}, []),
    ("QPAL_GEMM_MIN_BATCH=2", {"QPAL_GEMM_MIN_BATCH": "2"}, ["--reduced"]),
    ("QPAL_GEMM_MIN_BATCH=128", {"QPAL_GEMM_MIN_BATCH": "128"}, ["--reduced"]),
    ("QPAL_SHARE=0", {"QPAL_SHARE": "0"}, ["--reduced"]),
    ("QPAL_PAIR=0", {"QPAL_PAIR": "0"}, ["--reduced"]),
    ("QPAL_FORCE_G=2 QPAL_FORCE_RG=3", {"QPAL_FORCE_G": "2", "QPAL_FORCE_RG": "3"}, ["--reduced"]),
]


def build(workdir, capi=None):
    """hipcc --cuda-host-only: the two translation units side by side, then a link without the HIP runtime (the program's own
    stubs stand in for the memsets)."""
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-std=c++20", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Wno-unused-result"]
    units = [(capi or os.path.join(CSRC, "qpal_capi.hip"), "qpal_capi.o", "-O3"), (os.path.join(ROOT, "tests", "capi_trace.hip"), "capi_trace.o", "-O1")]
    procs = [subprocess.Popen([HIPCC, *flags, opt, "-c", src, "-o", os.path.join(workdir, obj)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for src, obj, opt in units]
    for p, (src, _, _) in zip(procs, units):
        out, _ = p.communicate()
        assert p.returncode == 0, f"{src} does not compile host-only:\n{out}"
    exe = os.path.join(workdir, "capi_trace")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-no-hip-rt", *[os.path.join(workdir, obj) for _, obj, _ in units], "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _env(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QPAL_")}
    env.update(knobs)
    return env


def run_all(exe):
    """-> {section: [lines]}, the runs side by side"""
    procs = [(name, subprocess.Popen([exe, *args], env=_env(knobs), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
             for name, knobs, args in RUNS]
    got = {}
    for name, p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, f"capi_trace [{name}] ended with {p.returncode}:\n{err[-2000:]}"
        got[name] = out.splitlines()
    return got


def show(exe, section, ids):
    """the arguments and the recorded calls of some cases of one run"""
    name, knobs, args = next(r for r in RUNS if r[0] == section)
    r = subprocess.run([exe, *args, "--show", ",".join(ids)], env=_env(knobs), capture_output=True, text=True, timeout=300)
    keep, on = [], False
    for line in r.stdout.splitlines():
        if not line.startswith(" "):
            on = line.split(" ")[0] in ids
        if on:
            keep.append(line)
    return "\n".join(keep)


def read_golden(path=GOLDEN):
    want, section = {}, None
    for line in open(path).read().splitlines():
        if line.startswith("[") and line.endswith("]"):
            section = line[1:-1]
            want[section] = []
        elif line and not line.startswith("#"):
            want[section].append(line)
    return want


def compare(exe, got, want, limit=4):
    """-> '' or a report: per section the cases whose line differs, the first few with their arguments and new trace"""
    report = []
    for name, _, _ in RUNS:
        g, w = got[name], want.get(name, [])
        wd = {l.split(" ")[0]: l for l in w}
        bad = [l for l in g if wd.get(l.split(" ")[0]) != l]
        if len(g) != len(w):
            report.append(f"[{name}] {len(g)} cases, the golden file has {len(w)}")
        if bad:
            report.append(f"[{name}] {len(bad)} of {len(g)} cases differ (id, return code, digest):")
            report += [f"  now  {l}\n  want {wd.get(l.split(' ')[0], '(no such case)')}" for l in bad[:limit]]
            report.append(show(exe, name, [l.split(" ")[0] for l in bad[:limit]]))
    return "\n".join(report)


def main(argv):
    import tempfile
    capi = argv[argv.index("--capi") + 1] if "--capi" in argv else None
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, capi)
        got = run_all(exe)
        again = run_all(exe)
        assert got == again, "two runs of one build differ"
        if "--check" in argv:
            report = compare(exe, got, read_golden())
            print(report or "capi_trace: every case as in the golden file")
            return 1 if report else 0
        with open(GOLDEN, "w") as f:
            f.write("# tests/capi_trace.hip: <case id> <return code> <FNV-1a digest of the case's recorded calls>, per run.\n"
                    "# Recorded by tests/golden/make_golden_capi_trace.py; not to be re-recorded by a refactor of the host path.\n")
            for name, _, _ in RUNS:
                f.write(f"[{name}]\n" + "\n".join(got[name]) + "\n")
        print(f"wrote {GOLDEN}: " + ", ".join(f"{len(got[n])} cases [{n}]" for n, _, _ in RUNS))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
