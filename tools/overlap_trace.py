"""Which kernels of one C2 fit run beside each other?  From a rocprofv3 --kernel-trace CSV (kernel trace alone, no counters):
the last complete fit, and for every kernel fit() queues on the engine's side stream the kernels
whose intervals overlap its own, with the hardware queue of each.  usage: overlap_trace.py <kernel_trace.csv> [--all]"""
import csv
import sys

SIDE = ("k_comp_count", "k_comp_fill", "k_scan_one", "k_comp_vals", "k_tr_steps")


def short(name):
    return name.replace("void ", "").split("(")[0][:44]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")) for r in rows)
    # one k_sid launch per fit: the last complete fit of the headline kind -- Levenshtein launches and the legacy draw's trace
    # (bench.py --full fits the sampler plugin and other workloads behind it) -- from its k_sid to the next fit's
    sid = [i for i, e in enumerate(ev) if e[2].startswith("k_sid")]
    fits = [ev[a:b] for a, b in zip(sid, sid[1:]) if all(any(e[2].startswith(k) for e in ev[a:b]) for k in ("k_lev", "k_tr_chase"))]
    fit = fits[-1]
    nn = [i for i, e in enumerate(fit) if e[2].startswith("k_get_nn")]
    if nn:
        fit = fit[:nn[0] + 1]   # (the graph kernel ends the fit; the benchmark's checks and the next fit's anchor rounds follow)
    t0 = fit[0][0]
    busy_end, busy = fit[0][0], 0
    for s, e, _, _ in fit:
        if e > busy_end:
            busy += e - max(s, busy_end)
            busy_end = e
    print("kernels %d, span %.3f ms, device busy %.3f ms, sum of kernel times %.3f ms, queues %s"
          % (len(fit), (fit[-1][1] - t0) / 1e6, busy / 1e6, sum(e - s for s, e, _, _ in fit) / 1e6, sorted({q for _, _, _, q in fit})))
    show_all = "--all" in sys.argv
    for i, (s, e, n, q) in enumerate(fit):
        side = n.startswith(SIDE)
        if not (side or show_all):
            continue
        beside = [(s2, e2, n2, q2) for j, (s2, e2, n2, q2) in enumerate(fit) if j != i and s2 < e and e2 > s]
        print("%9.1f .. %9.1f us  q%-3s %-44s %s" % ((s - t0) / 1e3, (e - t0) / 1e3, q, n, "" if beside else "alone"))
        for s2, e2, n2, q2 in beside:
            print("%25s beside q%-3s %-40s %9.1f .. %9.1f us (%5.1f us shared)"
                  % ("", q2, n2, (s2 - t0) / 1e3, (e2 - t0) / 1e3, (min(e, e2) - max(s, s2)) / 1e3))


if __name__ == "__main__":
    main()
