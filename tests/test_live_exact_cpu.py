"""The premises of tests/test_gpu_live_exact.py, checked without a GPU (oracle/live_exact.py).

The GPU file asserts that the lean live frame (csrc/rc_live.hip) and the frame-stepped plan give the same BITS on a state dict
whose linear2 rows hold one +-2^e each. Here, on the float32 CPU oracle's run of the same scripted cases:
  a. every linear2 of every row-frame is the same bits in index order, reversed, pairwise and in the lean order of both tile
     widths -- the premise;
  b. the LSTMs are not idle at the chosen gain (gate pre-activations beyond |2| and within |0.1|, |h| >= 0.3, all finite);
  c. the scripts visit every regime, idle rnn4 / rnn6 rows, deferred steps riding lean frames, init_net and transition frames;
  d. equality CAN fail: each wrong variant of the lean sums, of a layer step and of the fuse changes an output bit on a named case.
Run with -s for the figures."""
import numpy as np
import pytest
import torch

from oracle import live_exact as X

CASES = {c.name: c for c in X.CASES}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs(synth_assets):
    """{case: dict(steps, frames, lin2 {net: (W2, b2)})}: the float32 oracle on every case, once."""
    out = {}
    for case in X.CASES:
        sd = X.exact_sum_state_dict(X.WEIGHT_SEED, X.GAIN, case.pick)
        steps, frames = X.oracle_run(case, synth_assets["body"], sd)
        out[case.name] = dict(steps=steps, frames=frames, lin2={n: (sd[f"{n}.linear2.weight"], sd[f"{n}.linear2.bias"]) for n in X.NET_NAMES})
        del sd
    return out


def stacked(run, net):
    """(h [N, H], y [N, out], h_prev [N, H]) over every row-frame on which `net` stepped; h_prev: what the same row's linear2 read
    on its previous step (zeros before the first)."""
    hs, ys, prev, last = [], [], [], {}
    for s in run["steps"]:
        if s.net != net:
            continue
        for k, r in enumerate(s.rows):
            hs.append(s.h1[k]), ys.append(s.y[k]), prev.append(last.get(int(r), np.zeros_like(s.h1[k])))
            last[int(r)] = s.h1[k]
    return np.stack(hs), np.stack(ys), np.stack(prev)


# ---------------------------------------------------------------------------------------------------------------- the dict itself
def test_the_picks_reach_every_edge_of_the_sums():
    for net in X.NET_NAMES:
        H, out, _, S = X.geometry(net)
        chosen = set()
        for c in X.CASES:
            u = X.pick_units(net, c.pick)
            assert len(u) == out and all(0 <= v < H for v in u), (net, c.name)
            chosen |= set(u)
        assert set(X.required_units(net)) <= chosen, (net, sorted(set(X.required_units(net)) - chosen))
        assert {0, H - 1, 3, 4, 7, 8} <= chosen and {v % 8 for v in chosen} == set(range(8)), net
        for ut in (4, 8):
            nt = H // ut
            tiles = {v // ut for v in chosen}
            assert {S - 1, S, nt - 1} <= tiles, (net, ut)
            assert any(t % S == S - 1 and t + S >= nt for t in tiles), (net, ut)        # the last tile of the last slice
            assert any(t // S == -(-nt // S) - 1 for t in tiles), (net, ut)             # the largest q of the sum
        if out > 4:                                                                        # wide outputs: the tiles as far as the rows reach
            nt4 = H // 4
            first = {v // 4 for v in X.pick_units(net, 0)}
            assert set(range(min(out, nt4))) <= first, net
            assert {v // 4 for v in chosen} == set(range(nt4)), net                        # ... and every tile across the cases
    sd = X.exact_sum_state_dict(X.WEIGHT_SEED, X.GAIN, 3)
    for net in X.NET_NAMES:
        w = sd[f"{net}.linear2.weight"]
        assert ((w != 0).sum(axis=1) == 1).all() and set(np.abs(w[w != 0]).tolist()) <= {0.5, 1.0, 2.0}, net
    w7 = sd["rnn7.linear2.weight"]
    assert (w7 < 0).any() and (w7 > 0).any() and {0.5, 1.0, 2.0} == set(np.abs(w7[w7 != 0]).tolist())


# ------------------------------------------------------------------------------------------------------------ a. order independence
@pytest.mark.parametrize("name", list(CASES))
def test_every_summation_order_gives_the_same_bits(name, runs):
    run = runs[name]
    for net in X.NET_NAMES:
        W2, b2 = run["lin2"][net]
        h, y, _ = stacked(run, net)
        nz = np.abs(h[h != 0])
        assert np.isfinite(h).all() and nz.min() >= np.finfo(np.float32).tiny, (name, net, nz.min())   # no subnormal h: 2^-1 h is exact
        ref = bits(y)                                                                      # the oracle's own linear2 (its BLAS' order)
        orders = X.sum_orders(W2, b2, h)
        orders["lean UT=4"] = X.lean_linear2(W2, b2, h, net, 4)
        orders["lean UT=8"] = X.lean_linear2(W2, b2, h, net, 8)
        for k, v in orders.items():
            assert np.array_equal(bits(v), ref), (name, net, k, int((bits(v) != ref).sum()))
        u = np.asarray(X.pick_units(net, CASES[name].pick))                                # ... and it IS fl(+-2^e h[u(o)] + b[o])
        w = W2[np.arange(len(u)), u]
        assert np.array_equal(bits((w[None] * h[:, u]).astype(np.float32) + b2), ref), (name, net)


# ------------------------------------------------------------------------------------------------------- b. the LSTMs are not idle
def test_the_lstms_work_on_the_curved_part_of_their_gates(runs):
    for name in ("aql_b1", "aql_b4"):
        assert CASES[name].full
        for net in X.NET_NAMES:
            steps = [s for s in runs[name]["steps"] if s.net == net]
            g = np.abs(np.concatenate([np.concatenate([s.gates[0].ravel(), s.gates[1].ravel()]) for s in steps]))
            hmax = max(float(np.abs(s.hn).max()) for s in steps)
            print(f"{name} {net}: |gate| {g.min():.2e} .. {g.max():.3g} ({(g > 2).mean():.1%} beyond 2, {(g < 0.1).mean():.1%} within 0.1), max |h| {hmax:.3f}")
            assert np.isfinite(g).all(), (name, net)
            assert g.max() > 2.0 and g.min() < 0.1 and hmax >= 0.3, (name, net, g.max(), g.min(), hmax)
            assert g.max() < 16.0, (name, net)                 # ... nor saturated: from ~16.6 on a float32 sigmoid is 1.0 and forgets its sum


# ------------------------------------------------------------------------------------------------------------------- c. the census
def test_the_scripts_visit_every_branch_of_the_live_session(runs):
    n = dict(low=0, mid=0, high=0, idle=0, ride=0, init_net=0, transition=0, lean=0, frames=0)
    for name, run in runs.items():
        plan = X.plan_of_frames(run["frames"])
        for f, p in zip(run["frames"], plan):
            for k, code in (("low", 0), ("mid", 1), ("high", 2)):
                n[k] += int((f["regime"] == code).sum())
            for k in ("idle", "ride", "init_net", "transition"):
                n[k] += int(p[k].sum())
            n["lean"] += int(p["lean"])
            n["frames"] += 1
        # the device's rule leaves most of every script on the lean plan (the host's conservative mirror takes a few more frames off)
        assert sum(p["lean"] for p in plan) >= 0.75 * len(plan), name
        if CASES[name].B == 4:
            assert any(len(set(f["regime"].tolist())) == 3 for f in run["frames"]), name
        if CASES[name].B >= 2:                                                            # rows differ: some frame steps rnn4 on a part of the rows
            assert any(0 < int(p["idle"].sum()) < CASES[name].B for p in plan) or any(0 < int(p["ride"].sum()) < CASES[name].B for p in plan), name
    print("census (row-frames over the case set):", n)
    for k in ("low", "mid", "high", "idle", "ride", "init_net", "transition"):
        assert n[k] >= 10, (k, n)


# ------------------------------------------------------------------------------------------------------------------ d. sensitivity
def _visible_units(mut, net, ut):
    """the hidden units whose selection makes `mut` visible in net's sum at tile width ut"""
    H, _, _, S = X.geometry(net)
    nt = H // ut
    tile = {"tile 0 left out": 0, "last tile left out": nt - 1, "tile S left out": S, "a tile added twice": 1, "a stale partial taken": 0}.get(mut)
    if tile is not None:
        return range(tile * ut, (tile + 1) * ut)
    if mut == "unit index off by one inside a tile":
        return range(H)
    return range(H // 2, H)                                   # the tiles the other width's count drops, or reads without their being written


@pytest.mark.parametrize("mut", X.MUTATIONS)
def test_a_wrong_lean_sum_changes_a_bit(mut, runs):
    """every net, both tile widths: on the first case whose pick selects a unit the mutation touches, the output differs in at
    least one bit on at least one row-frame"""
    for net in X.NET_NAMES:
        for ut in (4, 8):
            if mut == "tile count of UT = 4 on UT = 8 partials" and ut == 4:
                continue
            vis = _visible_units(mut, net, ut)
            name = next((c.name for c in X.CASES if any(u in vis for u in X.pick_units(net, c.pick))), None)
            assert name is not None, (mut, net, ut)
            W2, b2 = runs[name]["lin2"][net]
            h, y, prev = stacked(runs[name], net)
            if mut in ("a stale partial taken", "tile count of UT = 4 on UT = 8 partials"):
                keep = np.abs(prev).max(axis=1) > 0                                        # (a row's first step has nothing stale to take)
                h, y, prev = h[keep], y[keep], prev[keep]
            got = X.lean_linear2(W2, b2, h, net, ut, mut, h_stale=prev)
            changed = int((bits(got) != bits(y)).any(axis=1).sum())
            if mut == "tile count of the other width" and ut == 8:
                # the H / 4 count on a buffer that only ever held H / 8 tiles adds the zeros the allocation was filled with: invisible by
                # construction, on the device as here -- it shows once the upper half holds anything (the mutation after this one)
                assert changed == 0, (net, changed)
                continue
            print(f"{mut}: {net} UT={ut} on {name}: {changed} of {len(h)} row-frames change")
            assert changed > 0, (mut, net, ut, name)


def test_a_wrong_layer_step_or_fuse_changes_a_bit(runs, synth_assets):
    """the recurrent half read from copy (st + 1) % 3 (the h of two steps ago) instead of (st + 2) % 3, and chunk Qw - 1 of a wave
    skipped: layer 1 of rnn2 on aql_b1 in the float32 restatement of live_lstm_body's K split; fmaf in the fuse's three-term product
    on aql_b4"""
    from robustcap_amd import synth
    sd = synth.make_state_dict(X.WEIGHT_SEED, X.GAIN)
    Wih, Whh = sd["rnn2.rnn.weight_ih_l1"], sd["rnn2.rnn.weight_hh_l1"]
    bias = (sd["rnn2.rnn.bias_ih_l1"] + sd["rnn2.rnn.bias_hh_l1"]).astype(np.float32)
    del sd
    steps = [s for s in runs["aql_b1"]["steps"] if s.net == "rnn2"]
    Qw = 2 * 512 // 64
    n_stale = n_skip = n = 0
    for k in range(2, len(steps), 4):
        s = steps[k]
        args = (Wih, Whh, bias, s.hn[0, 0])
        h, c = X.layer_step_f32(*args, s.hp[1, 0], s.cp[1, 0])
        # the restatement is the oracle's layer step up to the order of a 1024-term float32 sum (gate sums of size <= 16: 1e-5 of slack)
        assert np.abs(h - s.hn[1, 0]).max() <= 1e-5, (k, np.abs(h - s.hn[1, 0]).max())
        h_st, _ = X.layer_step_f32(*args, steps[k - 1].hp[1, 0], s.cp[1, 0])
        h_sk, _ = X.layer_step_f32(*args, s.hp[1, 0], s.cp[1, 0], skip=(2, Qw - 1))
        n_stale += int((bits(h_st) != bits(h)).any())
        n_skip += int((bits(h_sk) != bits(h)).any())
        n += 1
    print(f"h copy (st + 1) % 3 read: rnn2 layer 1 on aql_b1: {n_stale} of {n} row-frames change; chunk Qw - 1 of wave 2 skipped: {n_skip} of {n}")
    assert n_stale > 0 and n_skip > 0
    changed = total = 0
    for f in runs["aql_b4"]["frames"]:
        rows = f["regime"] > 0
        a, b = X.fuse_f32(f["j3dc"], f["Rcr"]), X.fuse_f32(f["j3dc"], f["Rcr"], fused=True)
        changed += int((bits(a) != bits(b)).any(axis=1)[rows].sum())
        total += int(rows.sum())
    print(f"fmaf in the fuse's three-term product: aql_b4: {changed} of {total} row-frames change")
    assert changed > 0
