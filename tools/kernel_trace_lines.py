"""kernel_trace.csv of `rocprofv3 --kernel-trace --output-format csv -d <dir>` -> one line per kernel of the diagonal E-step,
in start order: name, grid in work-items (x, y), workgroup size, static LDS bytes.
Usage: python tools/kernel_trace_lines.py <dir> <out.txt>"""
import csv
import glob
import re
import sys

paths = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
assert len(paths) == 1, paths
rows = list(csv.DictReader(open(paths[0])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
keep = [r for r in rows if re.search(r"estep|gmmmap_group", r["Kernel_Name"])]
def col(r, *names):
    for n in names:
        if n in r:
            return r[n]
    return "?"
with open(sys.argv[2], "w") as f:
    for r in keep:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        name = re.sub(r"\(.*$", "", name).replace("vcmi::", "")
        f.write("%s grid=%sx%s wg=%s lds=%s\n" % (name, col(r, "Grid_Size_X"), col(r, "Grid_Size_Y"), col(r, "Workgroup_Size_X"), col(r, "LDS_Block_Size", "LDS_Block_Size_v")))
print(len(rows), "kernels,", len(keep), "kept; columns:", ",".join(rows[0].keys()))
