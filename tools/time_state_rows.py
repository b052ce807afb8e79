"""Times kmpc_state_transfer against the only thing that moved trajectories before it, state_dict() + load_state_dict(), for the cfg2
dimension set (L = 20, N = 20, float64, MLP lift) -- the record in profiles/state_rows.txt.

    python tools/time_state_rows.py [--batch 4096] [--reps 200] [--kernels-only]

Legs: 4096 -> 4096 with a random permutation on both sides, 4096 -> 2048 (a random half into a whole handle).  Device events around
`reps` calls give the time of a CALL (validation kernels, the read-back of the status word and the host side included).  The time of the
two copy kernels alone comes from a kernel trace of this script in a run of its own (--kernels-only does nothing but the calls):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_state_rows.py --kernels-only
Bytes moved by the two copy kernels: 2 x row_elems x sizeof(T) x count (each row is read once and written once by each of them).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "koopman-online-updated-mpc_amd")]

HBM_PEAK_GBS = 8000.0  # (the figure bench.py uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from koopmpc import KoopmanMPC
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    B, L, N = args.batch, 20, 20
    w = random_mlp_weights(2, 100, 3, L, seed=2024)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))

    def make(batch):
        return KoopmanMPC(n=2, L=L, N=N, batch=batch, weights=w)

    src = make(B)
    src.set_model(*offline_edmd(lambda X: src.Encoder(X), plant=duffing_rk4))
    X = torch.tensor(initial_states(B, seed=3), dtype=torch.float64, device="cuda:0")
    src.rollout("duffing", X, r, 6)  # (a running estimator: have_prev = 1, every trajectory its own model)
    dst, half = make(B), make(B // 2)
    dst.load_state_dict(src.state_dict())  # (the same flags as src: a partial scatter is allowed)
    rng = np.random.RandomState(0)
    dev = "cuda:0"
    perm_s = torch.tensor(rng.permutation(B), dtype=torch.int32, device=dev)
    perm_d = torch.tensor(rng.permutation(B), dtype=torch.int32, device=dev)
    pick = torch.tensor(rng.permutation(B)[:B // 2], dtype=torch.int32, device=dev)
    ne = src.state_row_elems()
    legs = [("%d -> %d, random permutation" % (B, B), lambda: dst.transfer_state(src, src_idx=perm_s, dst_idx=perm_d), B),
            ("%d -> %d, random half" % (B, B // 2), lambda: half.transfer_state(src, src_idx=pick), B // 2)]
    print("cfg2 set: L = %d, N = %d, float64; row_elems = %d (%d bytes per row)" % (L, N, ne, 8 * ne))
    for name, call, count in legs:
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        if args.kernels_only:
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        moved = 2.0 * ne * 8 * count
        print("kmpc_state_transfer %-34s %9.1f us per call (device events, %d calls; validation and status read-back included): "
              "%.1f MB by the copy kernels, %.0f GB/s over the whole call = %.3f of %.0f GB/s"
              % (name, 1e3 * ms, args.reps, moved / 1e6, moved / (ms * 1e-3) / 1e9, moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, HBM_PEAK_GBS))
    if args.kernels_only:
        return
    # what a user could do before: the blob through the host, whole handles of one batch only
    for _ in range(2):
        dst.load_state_dict(src.state_dict())
    torch.cuda.synchronize()
    reps = max(3, args.reps // 10)
    t0 = time.perf_counter()
    for _ in range(reps):
        dst.load_state_dict(src.state_dict())
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / reps
    print("state_dict() + load_state_dict()  %d trajectories, same batch only %9.1f us per pair (host clock behind a device synchronise, %d pairs; "
          "blob of %.1f MB through host memory)" % (B, 1e3 * ms, reps, src.lib.kmpc_state_bytes(src.h) / 1e6))
    # the same hand-over on the device: state_to() / state_from() with a device blob
    blob = src.state_to()
    for _ in range(2):
        dst.state_from(src.state_to(blob))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        dst.state_from(src.state_to(blob))
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / reps
    print("state_to() + state_from()         %d trajectories, device blob      %9.1f us per pair (host clock, %d pairs)" % (B, 1e3 * ms, reps))


if __name__ == "__main__":
    main()
