"""Per-step kernel time by category from ``rocprofv3 --kernel-trace --stats`` runs of ``tools/bench_stages.py --only STATE``:
weight gradients, weight re-packs, AdamW and everything else, and the launches that differ between two states.

    python tools/stage_kernel_split.py STEPS none_kernel_stats.csv transfer_kernel_stats.csv

STEPS: training steps each profiled run executed (warm-up steps + replays)."""
import csv
import sys

CATEGORIES = (("weight gradient", ("wgrad", "upcat_chain", "border_sums")), ("weight re-pack", ("wpack", "weight_pack", "upcat_compose")),
              ("AdamW", ("adamw",)))


def category(name):
    low = name.lower()
    for cat, keys in CATEGORIES:
        if any(k in low for k in keys):
            return cat
    return "other"


def load(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def main(steps, path_a, path_b):
    a, b = load(path_a), load(path_b)
    for tag, table in (("A", a), ("B", b)):
        cats = {}
        for name, (calls, ns) in table.items():
            c = cats.setdefault(category(name), [0, 0.0])
            c[0] += calls
            c[1] += ns
        total = sum(v[1] for v in cats.values())
        print(f"{tag}: {total / steps / 1e6:.3f} ms of kernels per step, {sum(v[0] for v in cats.values()) / steps:.1f} launches per step")
        for cat, (calls, ns) in sorted(cats.items(), key=lambda kv: -kv[1][1]):
            print(f"   {cat:16s} {ns / steps / 1e6:8.3f} ms  {calls / steps:7.1f} launches per step")
    print("launches per step that differ (A -> B), ms per step:")
    for name in sorted(set(a) | set(b), key=lambda n: -abs(a.get(n, (0, 0.0))[1] - b.get(n, (0, 0.0))[1])):
        (ca, ta), (cb, tb) = a.get(name, (0, 0.0)), b.get(name, (0, 0.0))
        if ca != cb:
            print(f"   {ca / steps:6.1f} -> {cb / steps:6.1f}  {ta / steps / 1e6:7.3f} -> {tb / steps / 1e6:7.3f} ms  [{category(name)}] {name[:110]}")


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2], sys.argv[3])
