"""Who runs while no field kernel does: from a rocprofv3 --kernel-trace CSV, the wall time during which at least one
kernel executes, the part of it during which no field kernel executes, and that part attributed to the kernels that
execute then (a moment shared by k of them counts 1/k for each).  usage: trace_outside_field.py <dir|csv> [skip_ms]
skip_ms = leading milliseconds of the trace to leave out (set-up and warm-up), default 0."""
import collections, csv, glob, os, re, sys
path = sys.argv[1]
files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)) if os.path.isdir(path) else [path]
if len(files) != 1:       # one process, one trace: several would be several runs' clocks on one time line
    sys.exit(f"{path}: {len(files)} *kernel_trace.csv files, need exactly one" + "".join("\n  " + f for f in files))
rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))]
if not rows:
    sys.exit(f"{files[0]}: no dispatches")
t_first = min(s for s, _, _ in rows) + int(float(sys.argv[2]) * 1e6 if len(sys.argv) > 2 else 0)
rows = [r for r in rows if r[0] >= t_first]
is_field = lambda n: "field_kernel" in n or "field_half_kernel" in n
short = lambda n: re.sub(r"\(.*$", "", n.replace("void ", "").replace("ced::", ""))[:70]
ev = []
for s, e, n in rows:
    ev.append((s, 1, n)); ev.append((e, -1, n))
ev.sort(key=lambda x: (x[0], x[1]))
running = collections.Counter()
n_field = 0
busy = outside = 0
share = collections.Counter()
prev = ev[0][0]
for t, kind, n in ev:
    dt = t - prev
    k = sum(running.values())
    if dt > 0 and k > 0:
        busy += dt
        if n_field == 0:
            outside += dt
            for name, c in running.items():
                if c: share[name] += dt * c / k
    prev = t
    running[n] += kind
    if is_field(n): n_field += kind
span = ev[-1][0] - ev[0][0]
print(f"{len(rows)} dispatches over {span / 1e6:.1f} ms; a kernel executes during {busy / 1e6:.1f} ms, "
      f"no field kernel during {outside / 1e6:.2f} ms of that ({100.0 * outside / busy:.1f} %)")
calls = collections.Counter(n for _, _, n in rows)
tot = collections.Counter()
for s, e, n in rows: tot[n] += e - s
for name, v in share.most_common(12):
    print(f"  {100.0 * v / busy:5.2f} % of kernel-executing wall  {v / 1e6:8.3f} ms outside the field kernel, "
          f"{tot[name] / 1e6:8.3f} ms in all, {calls[name]:6d} calls  {short(name)}")
