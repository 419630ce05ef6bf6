#!/usr/bin/env python3
"""Same-calls check of the entries that stage a host-built table (csrc/rc_internal.h: StagedTable), between two builds of the library.

    rocprofv3 --hip-trace --kernel-trace -f rocpd -d DIR_A -o a -- python tools/staged_tables_same_calls.py run OUT_A.npz   (RC_LIB_PATH: the parent's build = A)
    rocprofv3 --hip-trace --kernel-trace -f rocpd -d DIR_B -o b -- python tools/staged_tables_same_calls.py run OUT_B.npz
    python tools/staged_tables_same_calls.py compare DIR_A DIR_B OUT_A.npz OUT_B.npz

run: three calls of each of the eight entries on a context each -- the cases of tests/test_gpu_staged_tables.py, calls 0 .. 2 (tables of 1,
3 and 2 entries: the device table grows at the first two calls and is reused at the third) -- and every output saved as its bits.
compare: the HIP API calls of the issuing thread as (name, stream arguments, event arguments), handles replaced by their order of first
appearance (a destroyed handle's address counts anew), hipStreamQuery left out; the kernels per stream as (name, grid, workgroup); the
outputs. The same once more with the allocation, creation and destruction calls left out."""
import glob
import itertools
import os
import sqlite3
import sys
from collections import Counter, defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import test_gpu_staged_tables as S
    from robustcap_amd import synth

    saved, case = {}, [None]

    def drive(make, call):
        ctx = make()
        torch.cuda.synchronize()
        outs = [call(ctx, k) for k in range(3)]
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            for i, a in enumerate(o):
                saved[f"{case[0]}_{k}_{i}"] = a.detach().cpu().contiguous().view(-1).view(torch.int32).numpy()
        del ctx, outs
        torch.cuda.synchronize()

    S._drive = drive
    assets = {"state_dict": synth.make_state_dict(0), "body": synth.make_body(1)}
    for name in ("subnet_eval", "motion_metrics_no_mesh", "prepare_motions", "subnet_batch", "subnet_batch_parts", "subnet_corpus", "subnet_forward"):
        case[0] = name
        getattr(S, "test_" + name)()
    case[0] = "sequence_rows"
    S.test_sequence_rows(assets)
    np.savez(out, **saved)
    print("saved", len(saved), "arrays to", out, flush=True)


def tab(cur, prefix):
    names = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    return next(t for t in names if t.startswith(prefix))


def load(path):
    db = sqlite3.connect(path)
    cur = db.cursor()
    reg, st, arg, ev = tab(cur, "rocpd_region"), tab(cur, "rocpd_string"), tab(cur, "rocpd_arg"), tab(cur, "rocpd_event")
    rows = cur.execute(f"select r.id, r.tid, r.start, s.string, r.event_id, c.string from `{reg}` r join `{st}` s on r.name_id = s.id "
                       f"left join `{ev}` e on r.event_id = e.id left join `{st}` c on e.category_id = c.id order by r.start, r.id").fetchall()
    cats = Counter(r[5] for r in rows)
    rows = [r for r in rows if r[3].startswith("hip") and (r[5] is None or "HIP" in r[5].upper())]
    tid = Counter(r[1] for r in rows).most_common(1)[0][0]
    rows = [r for r in rows if r[1] == tid and r[3] != "hipStreamQuery"]
    args = defaultdict(list)
    for e, pos, typ, name, val in cur.execute(f"select event_id, position, type, name, value from `{arg}` order by event_id, position"):
        args[e].append((pos, typ, name, val))
    seen_s, seen_e = {}, {}
    cs, ce = itertools.count(), itertools.count()
    calls, compared = [], 0
    kinds = set()
    for _, _, _, name, eid, _ in rows:
        sa, ea = [], []
        for pos, typ, an, val in args.get(eid, []):
            kinds.add((typ, an))
            if name.startswith("hipEventCreate") or name.startswith("hipStreamCreate"):
                continue
            if an.lower() in ("stream", "hstream") or typ.strip() == "hipStream_t":
                sa.append(seen_s.setdefault(val, next(cs)))
            elif an.lower() in ("event", "start", "stop") or typ.strip() == "hipEvent_t":
                ea.append(seen_e.setdefault(val, next(ce)))
        compared += len(sa) + len(ea)
        calls.append((name, tuple(sa), tuple(ea)))
        if name in ("hipEventDestroy", "hipStreamDestroy"):          # the handle's address may be handed out again: a new event then
            for pos, typ, an, val in args.get(eid, []):
                (seen_e if name == "hipEventDestroy" else seen_s).pop(val, None)
    disp, sym = tab(cur, "rocpd_kernel_dispatch"), tab(cur, "rocpd_info_kernel_symbol")
    scol = [r[1] for r in cur.execute(f"pragma table_info(`{sym}`)")]
    ncol = "kernel_name" if "kernel_name" in scol else ("display_name" if "display_name" in scol else "name")
    ks = cur.execute(f"select d.stream_id, k.{ncol}, d.grid_size_x, d.grid_size_y, d.grid_size_z, d.workgroup_size_x, d.workgroup_size_y, "
                     f"d.workgroup_size_z from `{disp}` d join `{sym}` k on d.kernel_id = k.id order by d.dispatch_id").fetchall()
    per, order = defaultdict(list), {}
    for k in ks:
        per[order.setdefault(k[0], len(order))].append(k[1:])
    print('arg kinds:', sorted(k for k in kinds if 'tream' in k[0] + k[1] or 'vent' in k[0] + k[1]))
    return calls, compared, per, cats, len(ks)


def compare(dir_a, dir_b, out_a, out_b):
    import difflib
    pa = glob.glob(dir_a + "/**/*.db", recursive=True)[0]
    nb = glob.glob(dir_b + "/**/*.db", recursive=True)[0]
    A, ca, ka, cats, na = load(pa)
    B, cb, kb, _, nk = load(nb)
    print("categories:", dict(cats))
    print(f"HIP API calls: parent {len(A)}, new {len(B)}; stream / event arguments compared {ca} | {cb}")
    print("names parent - new:", dict(Counter(a[0] for a in A) - Counter(b[0] for b in B)))
    print("names new - parent:", dict(Counter(b[0] for b in B) - Counter(a[0] for a in A)))
    if len(A) == len(B):
        diff = [i for i in range(len(A)) if A[i] != B[i]]
        print("differing positions:", len(diff))
        for i in diff[:60]:
            print("  ", i, A[i], "|", B[i])
    else:
        sm = difflib.SequenceMatcher(a=[str(x) for x in A], b=[str(x) for x in B], autojunk=False)
        for op, i1, i2, j1, j2 in sm.get_opcodes():
            if op != "equal":
                print("  ", op, i1, [A[i] for i in range(i1, i2)][:8], "->", j1, [B[j] for j in range(j1, j2)][:8])
    # the same with the allocation / creation calls taken out (they carry no stream or event argument that is compared)
    alloc = {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreateWithFlags", "hipEventCreate", "hipEventDestroy", "hipHostAlloc"}
    print("allocation / creation / destruction calls: parent", dict(Counter(a[0] for a in A if a[0] in alloc)), "| new", dict(Counter(b[0] for b in B if b[0] in alloc)))
    A2, B2 = [a for a in A if a[0] not in alloc], [b for b in B if b[0] not in alloc]
    print(f"without allocation / creation calls: parent {len(A2)}, new {len(B2)}, differing positions",
          sum(x != y for x, y in zip(A2, B2)) if len(A2) == len(B2) else "n/a (lengths differ)")
    if len(A2) != len(B2) or any(x != y for x, y in zip(A2, B2)):
        sm = difflib.SequenceMatcher(a=[str(x) for x in A2], b=[str(x) for x in B2], autojunk=False)
        for op, i1, i2, j1, j2 in sm.get_opcodes():
            if op != "equal":
                print("  ", op, i1, [A2[i] for i in range(i1, i2)][:8], "->", j1, [B2[j] for j in range(j1, j2)][:8])
    print(f"kernels: parent {na} on {len(ka)} streams, new {nk} on {len(kb)} streams; per-stream sequences identical:",
          len(ka) == len(kb) and all(ka[s] == kb[s] for s in ka))

    import numpy as np
    a, b = np.load(out_a), np.load(out_b)
    print("outputs:", len(a.files), "|", len(b.files), "arrays; same names:", sorted(a.files) == sorted(b.files), "; bitwise equal:",
          sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == "compare":
        compare(*sys.argv[2:6])
    else:
        sys.exit(__doc__)
