#!/usr/bin/env python3
"""Development: how the exchange fetch rounds of k_cl_run are issued, read from the device assembly that
`hipcc ... -save-temps=obj` leaves beside the library (potus_hmc-hip-amdgcn-amd-amdhsa-gfx950.s).
    python scripts/dev/fetch_issue_table.py path/to/device.s [K ...]        (default K: 16)
Inside a kernel's text (between its label and its .size line) the script looks at two kinds of lines only: the 128-bit buffer loads
(`buffer_load_dwordx4`, every exchange word is one) and `s_waitcnt` with a vmcnt field.  Loads that follow each other within GAP lines
form a group; a group of NB loads is a round of xld<NB>.  For every group it prints the number of loads and every vmcnt wait that sits
between the first and the last load, as "vmcnt(N) after i loads" -- VMEM returns in order, so such a wait holds the remaining loads back
until load i - 1 - N has returned.  A round issued back to back prints "none".  The words "each load followed by vmcnt(0)" mark the
shape of a re-fetch loop whose loads sit under one branch each."""
import re
import sys

GAP = 40


def kernels(path):
    name, start, body = None, 0, []
    for no, line in enumerate(open(path, errors="replace"), 1):
        if name is None:
            m = re.match(r"(_Z\d+k_cl_runILi(\d+)ELb([01])E\w*):", line)
            if m:
                name, start, body = (m.group(1), int(m.group(2)), m.group(3) == "1"), no, []
        elif line.startswith("\t.size\t" + name[0]):
            yield name[1], name[2], start, body
            name = None
        elif "buffer_load_dwordx4" in line:
            body.append((no, "L", line.split()[1].rstrip(",")))
        elif "s_waitcnt" in line and "vmcnt(" in line:
            body.append((no, "W", re.search(r"vmcnt\(\d+\)", line).group(0)))


def groups(body):
    loads = [i for i, e in enumerate(body) if e[1] == "L"]
    cur = []
    for i in loads:
        if cur and body[i][0] - body[cur[-1]][0] > GAP:
            yield cur
            cur = []
        cur.append(i)
    if cur:
        yield cur


def describe(body, g):
    waits, n = [], 0
    for i in range(g[0], g[-1] + 1):
        if body[i][1] == "L":
            n += 1
        else:
            waits.append((body[i][2], n))
    if not waits:
        return "none"
    if len(g) > 2 and len(waits) == len(g) - 1 and all(w == ("vmcnt(0)", k + 1) for k, w in enumerate(waits)):
        return "each load followed by vmcnt(0)"
    return ", ".join(f"{w} after {n}" for w, n in waits)


if __name__ == "__main__":
    want = [int(a) for a in sys.argv[2:]] or [16]
    for K, twin, start, body in sorted(kernels(sys.argv[1]), key=lambda k: (k[0], k[1])):
        if K not in want:
            continue
        print(f"k_cl_run<{K}, {'true' if twin else 'false'}>   (lines counted from the kernel's label)")
        for g in groups(body):
            if len(g) < 2:
                continue
            print(f"  +{body[g[0]][0] - start:6d}  {len(g):2d} loads  first {body[g[0]][2]:10s} waits between first and last load: {describe(body, g)}")
