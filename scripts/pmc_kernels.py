"""Per-kernel means of rocprofv3 --pmc passes (csv output): for every kernel whose name holds one of the given
substrings, the dispatches seen and each counter's mean per dispatch, summed over the passes' directories.
Usage: python scripts/pmc_kernels.py <out.json> <kernel-substring>[,<substring>...] <pass_dir>..."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def main():
    out, subs, dirs = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
    res = defaultdict(dict)
    for d in dirs:
        tot, disp = defaultdict(float), defaultdict(set)
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row.get("Kernel_Name", "")
                if not any(s in name for s in subs):
                    continue
                name = name.replace("void ", "").split("(")[0]
                tot[(name, row["Counter_Name"])] += float(row["Counter_Value"])
                disp[name].add((f, row["Dispatch_Id"]))
        for (name, ctr), v in tot.items():
            res[name]["dispatches"] = len(disp[name])
            res[name][ctr] = v / len(disp[name])
    json.dump(res, open(out, "w"), indent=1, sort_keys=True)
    for name, r in sorted(res.items()):
        print(name, json.dumps(r, sort_keys=True))


if __name__ == "__main__":
    main()
