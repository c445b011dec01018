#!/usr/bin/env python3
"""Reduce a rocprofv3 --kernel-trace run of tests/test_gemm_layout_kernel.py to
the distinct GEMM kernel names with their launch counts, and hold them against
the routes of tests/gemm_layouts.py's cell table.

  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- \
      python -m pytest tests/test_gemm_layout_kernel.py -m gpu
  python scripts/gemm_layout_routes.py DIR profiles/gemm_layout_routes.json
"""
import csv
import json
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import gemm_layouts as gl  # noqa: E402

GEMM = re.compile(r"\bk_(gemm|gemm_wres|gemm_tn_big|sum_splits_\w+|split3_b|gemm3_\w+|s3_tn|x3_\w+)\b")


def norm(name):
    """`void nts_hip::k_gemm<false, 4, ...>(int, ...) [clone .kd]` -> `k_gemm<false, 4, ...>`"""
    name = re.sub(r"^void\s+", "", name.strip()).replace("nts_hip::", "")
    m = re.match(r"\w+", name)
    if not m:
        return name
    end = m.end()
    if name[end:end + 1] == "<":  # the template instance: up to its matching '>'
        depth = 0
        for j in range(end, len(name)):
            depth += {"<": 1, ">": -1}.get(name[j], 0)
            if depth == 0:
                end = j + 1
                break
    name = name[:end]
    name = re.sub(r"\(bool\)1", "true", re.sub(r"\(bool\)0", "false", name))
    name = re.sub(r"\((?:int|unsigned int)\)(\d+)", r"\1", name)
    return re.sub(r"\s*,\s*", ", ", name).strip()


def main(trace_dir, out):
    counts = {}
    for f in sorted(pathlib.Path(trace_dir).rglob("*kernel_trace.csv")):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                n = norm(row["Kernel_Name"])
                if GEMM.search(n):
                    counts[n] = counts.get(n, 0) + 1
    want = sorted({t for c in gl.CELLS for t in gl.trace_names(c.route)})
    missing = [t for t in want if t not in counts]
    extra = [n for n in sorted(counts) if n not in want]
    doc = {"source": "rocprofv3 --kernel-trace of tests/test_gemm_layout_kernel.py (one run)",
           "kernels": dict(sorted(counts.items())), "table_instances": len(want),
           "missing_from_trace": missing, "not_in_table": extra}
    pathlib.Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"distinct": len(counts), "missing": missing, "extra": extra}))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
