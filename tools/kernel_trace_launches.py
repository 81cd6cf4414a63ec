"""The launches of a ``rocprofv3 --kernel-trace`` run as an ordered list: for every dispatch, in dispatch order, one line

    <kernel name with its template arguments> grid=<x,y,z> workgroup=<x,y,z> lds=<bytes>

and, on the last line, the SHA-256 of the list.  Two builds whose lists are equal launch the same kernels on the same grids:
what a bitwise digest of the results (tools/vit_forward_digest.py) cannot see, since another tile shape can give the same bits.

    rocprofv3 --kernel-trace -f csv -d trace -- python tools/vit_forward_digest.py --only /h3/ > /dev/null
    python tools/kernel_trace_launches.py --match anyloc:: trace > launches.txt

Several CSV files (one per traced process) are taken in the order of their names."""
import argparse
import csv
import glob
import hashlib
import os


def launches(path, match=""):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {path}")
    out = []
    for f in files:
        with open(f, newline="") as fh:
            rows = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(fh)]
        rows.sort(key=lambda r: int(r["dispatch_id"]))
        for r in rows:
            if match in r["kernel_name"]:
                grid, wg = (",".join(r[f"{what}_size_{a}"] for a in "xyz") for what in ("grid", "workgroup"))
                out.append(f"{r['kernel_name']} grid={grid} workgroup={wg} lds={r['lds_block_size']}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", help="a kernel-trace CSV file, or a directory searched for *kernel_trace.csv")
    ap.add_argument("--match", default="", help="keep the kernels whose name contains this")
    args = ap.parse_args()
    lines = launches(args.trace, args.match)
    print("\n".join(lines))
    print("sha256 " + hashlib.sha256("\n".join(lines).encode()).hexdigest() + f" ({len(lines)} launches)")


if __name__ == "__main__":
    main()
