"""(kernel name, grid, workgroup size, LDS bytes) of every dispatch of a rocprofv3 kernel trace, in dispatch order, one line
per run of identical dispatches ("... xCOUNT"): the text two builds are compared by (profiles/README.md).  The runtime's
own copy and fill kernels (hipMemcpy / hipMemset[Async]: a plan's upload, the hand-off's flag reset) keep their place in
the sequence as "runtime copy/fill xCOUNT" lines, without their shapes.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/launch_sequence.py
    python profiles/tools/kernel_sequence.py DIR out.txt
"""
import csv
import glob
import sys


def main(trace_dir, out_path):
    files = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)
    assert len(files) == 1, files
    with open(files[0]) as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    lines, runtime = [], 0
    for r in rows:
        line = "%s grid %s,%s,%s wg %s,%s,%s lds %s" % (
            r["Kernel_Name"].split("(")[0].replace("void ", ""), r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
            r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], r["LDS_Block_Size"])
        if r["Kernel_Name"].startswith("__amd_rocclr_"):
            line, runtime = "runtime copy/fill", runtime + 1
        if lines and lines[-1][0] == line:
            lines[-1][1] += 1
        else:
            lines.append([line, 1])
    with open(out_path, "w") as out:
        out.write("# %d dispatches, %d of them copy / fill kernels of the runtime (no shapes listed)\n" % (len(rows), runtime))
        for line, n in lines:
            out.write("%s x%d\n" % (line, n))
    print(len(rows), "dispatches,", len(lines), "lines")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
