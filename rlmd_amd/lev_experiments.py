"""The reference's leverage experiments as host entry points (lev/coin_flip.py,
lev/dice_roll.py, lev/dice_roll_sh.py, lev/gbm.py).

Each driver takes the script's module constants as keyword defaults, runs its
input checks (rlmd_amd/config.py lev_*_tests), derives TOP and LEV_FACTOR as the
script does, draws the outcome matrix once on the device (lev.sample_outcomes,
seed 420), calls the sweeps of rlmd_amd/lev.py in the script's order, writes the
script's ``results/multiverse/*.npy`` files with its shapes and dtypes, logs the
``*_fixed_final_lev`` summaries and the ``TOTAL TIME`` line, and returns the
arrays.  Plotting (the reference's plotting/ package) is not part of the build.

    python -m rlmd_amd.lev_experiments coin_flip [--investors N --horizon T --out DIR --seed S]

Each driver also takes ``timings={}`` and fills it with every call's wall time in
milliseconds (the device synchronised before and after), ``total`` included.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import config, lev

EXPERIMENTS = ("coin_flip", "dice_roll", "dice_roll_sh", "gbm")


class _Run:
    """Shared bookkeeping of one experiment: timed calls, saved arrays, the log."""

    def __init__(self, path_results, device, log, timings):
        self.path, self.dev, self.log = path_results, torch.device(device), log
        self.timings = timings if timings is not None else {}
        self.arrays = {}
        os.makedirs(path_results, exist_ok=True)
        self.start = time.perf_counter()

    def call(self, name, fn, *args, **kw):
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        torch.cuda.synchronize(self.dev)
        self.timings[name] = (time.perf_counter() - t0) * 1e3
        return out

    def final(self, key, name, fn, *args):
        """A *_fixed_final_lev call: its summary lines go to the log, its statistics
        [n_lev, 13] into the returned arrays (the reference only prints them)."""
        stats, _ = self.call(name, fn, *args, verbose=self.log)
        self.arrays[key] = stats.cpu().numpy()

    def save(self, stem, tensor):
        a = tensor.cpu().numpy()
        np.save(os.path.join(self.path, stem + ".npy"), a)
        self.arrays[stem] = a

    def total(self):
        t = time.perf_counter() - self.start
        self.log("TOTAL TIME: {:1.0f}s = {:1.1f}m = {:1.2f}h".format(t, t / 60, t / 3600))
        self.timings["total"] = t * 1e3
        self.start = time.perf_counter()


def _top(top, investors):
    top = investors * 1e-4 if top is None else top
    return top, (int(top) if top > 1 else 1)  # minimum 1 person in the top sample


def _lev_factor(up_r, down_r, asym_lim):
    """coin_flip.py:145-152 / dice_roll.py:132-139: the leverage bound 1 / the bigger
    payoff, offset by ASYM_LIM, in the reference's f32 tensor arithmetic."""
    bigger = np.abs(down_r) if np.abs(up_r) >= np.abs(down_r) else -np.abs(up_r)
    lf = torch.tensor(1 / bigger)
    asym = torch.tensor(asym_lim)
    return lf - asym if np.abs(up_r) > np.abs(down_r) else lf + asym


def coin_flip(INVESTORS=1e6, HORIZON=3e3, TOP=None, VALUE_0=1e2, UP_PROB=0.5, UP_R=0.5, DOWN_R=-0.4, ASYM_LIM=1e-12,
              l0_l=0.05, l0_h=1.00, l0_i=0.05, l1_l=0.10, l1_h=1.00, l1_i=0.10,
              s2_l=0.10, s2_h=0.10, s2_i=0.10, r2_l=0.00, r2_h=0.00, r2_i=0.10,
              s3_l=0.05, s3_h=0.95, s3_i=0.05, r3_l=0.70, r3_h=0.95, r3_i=0.05,
              ru_l=0.20, ru_h=0.80, ru_i=0.001, rd_l=0.20, rd_h=0.80, rd_i=0.001, pu_l=0.25, pu_h=0.75, pu_i=0.25,
              path_results="./results/multiverse/", seed=420, device="cuda:0", log=print, timings=None):
    """lev/coin_flip.py: investors 1 (fixed leverages), 2 and 3 (stop-loss / retention)
    and 4 (the Kelly grid).  TOP defaults to INVESTORS * 1e-4."""
    TOP, top = _top(TOP, INVESTORS)
    config.lev_coin_tests(INVESTORS, HORIZON, TOP, VALUE_0, UP_PROB, UP_R, DOWN_R, ASYM_LIM, path_results, l0_l, l0_h,
                          l0_i, l1_l, l1_h, l1_i, s2_l, s2_h, s2_i, r2_l, r2_h, r2_i, s3_l, s3_h, s3_i, r3_l, r3_h,
                          r3_i, ru_l, ru_h, ru_i, rd_l, rd_h, rd_i, pu_l, pu_h, pu_i)
    log("Coin Flip Experiment Tests: Passed")
    inv, hor = int(INVESTORS), int(HORIZON)
    lev_factor = _lev_factor(UP_R, DOWN_R, ASYM_LIM)
    run = _Run(path_results, device, log, timings)
    dev = run.dev
    outcomes = run.call("sample_outcomes", lev.sample_outcomes, "coin", inv, hor, seed=seed, device=dev,
                        up_prob=UP_PROB)
    run.final("coin_final_stats", "coin_fixed_final_lev", lev.coin_fixed_final_lev, dev, outcomes, top, VALUE_0, UP_R,
              DOWN_R, l0_l, l0_h, l0_i)
    d, d_T = run.call("coin_smart_lev", lev.coin_smart_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R, DOWN_R, l1_l,
                      l1_h, l1_i)
    run.save("coin_inv1_val", d)
    run.save("coin_inv1_val_T", d_T)
    del d, d_T
    d = run.call("coin_big_brain_lev inv2", lev.coin_big_brain_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R,
                 DOWN_R, lev_factor, s2_l, s2_h, s2_i, r2_l, r2_h, r2_i)
    run.save("coin_inv2_val", d)
    d = run.call("coin_big_brain_lev inv3", lev.coin_big_brain_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R,
                 DOWN_R, lev_factor, s3_l, s3_h, s3_i, r3_l, r3_h, r3_i)
    run.save("coin_inv3_val", d)
    d = run.call("coin_galaxy_brain_lev", lev.coin_galaxy_brain_lev, dev, ru_l, ru_h, ru_i, rd_l, rd_h, rd_i, pu_l,
                 pu_h, pu_i)
    run.save("coin_inv4_lev", d)
    run.total()
    return run.arrays


def dice_roll(INVESTORS=1e6, HORIZON=5e3, TOP=None, VALUE_0=1e2, UP_PROB=1 / 6, DOWN_PROB=1 / 6, UP_R=0.5,
              DOWN_R=-0.5, MID_R=0.05, ASYM_LIM=1e-12,
              l0_l=0.05, l0_h=1.00, l0_i=0.05, l1_l=0.10, l1_h=1.00, l1_i=0.10,
              s2_l=0.10, s2_h=0.10, s2_i=0.10, r2_l=0.00, r2_h=0.00, r2_i=0.10,
              s3_l=0.05, s3_h=0.95, s3_i=0.05, r3_l=0.45, r3_h=0.95, r3_i=0.05,
              path_results="./results/multiverse/", seed=420, device="cuda:0", log=print, timings=None):
    """lev/dice_roll.py: the three-outcome die, investors 1, 2 and 3."""
    TOP, top = _top(TOP, INVESTORS)
    config.lev_dice_tests(INVESTORS, HORIZON, TOP, VALUE_0, UP_PROB, DOWN_PROB, UP_R, DOWN_R, MID_R, ASYM_LIM,
                          path_results, l0_l, l0_h, l0_i, l1_l, l1_h, l1_i, s2_l, s2_h, s2_i, r2_l, r2_h, r2_i, s3_l,
                          s3_h, s3_i, r3_l, r3_h, r3_i)
    log("Dice Roll Experiment Tests: Passed")
    inv, hor = int(INVESTORS), int(HORIZON)
    probs = (UP_PROB, DOWN_PROB, 1 - (UP_PROB + DOWN_PROB))
    lev_factor = _lev_factor(UP_R, DOWN_R, ASYM_LIM)
    run = _Run(path_results, device, log, timings)
    dev = run.dev
    outcomes = run.call("sample_outcomes", lev.sample_outcomes, "dice", inv, hor, seed=seed, device=dev, probs=probs)
    run.final("dice_final_stats", "dice_fixed_final_lev", lev.dice_fixed_final_lev, dev, outcomes, top, VALUE_0, UP_R,
              DOWN_R, MID_R, l0_l, l0_h, l0_i)
    d, d_T = run.call("dice_smart_lev", lev.dice_smart_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R, DOWN_R, MID_R,
                      l1_l, l1_h, l1_i)
    run.save("dice_inv1_val", d)
    run.save("dice_inv1_val_T", d_T)
    del d, d_T
    d = run.call("dice_big_brain_lev inv2", lev.dice_big_brain_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R,
                 DOWN_R, MID_R, lev_factor, s2_l, s2_h, s2_i, r2_l, r2_h, r2_i)
    run.save("dice_inv2_val", d)
    d = run.call("dice_big_brain_lev inv3", lev.dice_big_brain_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R,
                 DOWN_R, MID_R, lev_factor, s3_l, s3_h, s3_i, r3_l, r3_h, r3_i)
    run.save("dice_inv3_val", d)
    run.total()
    return run.arrays


def dice_roll_sh(INVESTORS=1e6, HORIZON=2e3, TOP=None, VALUE_0=1e2, UP_PROB=1 / 6, DOWN_PROB=1 / 6, UP_R=0.5,
                 DOWN_R=-0.5, MID_R=0.05, SH_UP_R=-1, SH_DOWN_R=5, SH_MID_R=-1,
                 l0_l=0.73, l0_h=1.00, l0_i=0.03, l1_l=0.73, l1_h=1.00, l1_i=0.03,
                 path_results="./results/multiverse/", seed=420, device="cuda:0", log=print, timings=None):
    """lev/dice_roll_sh.py: the die with its safe haven, investor 1."""
    TOP, top = _top(TOP, INVESTORS)
    config.lev_dice_sh_tests(INVESTORS, HORIZON, TOP, VALUE_0, UP_PROB, DOWN_PROB, UP_R, DOWN_R, MID_R, SH_UP_R,
                             SH_DOWN_R, SH_MID_R, path_results, l0_l, l0_h, l0_i, l1_l, l1_h, l1_i)
    log("Dice Roll (Safe Haven) Experiment Tests: Passed")
    inv, hor = int(INVESTORS), int(HORIZON)
    probs = (UP_PROB, DOWN_PROB, 1 - (UP_PROB + DOWN_PROB))
    run = _Run(path_results, device, log, timings)
    dev = run.dev
    outcomes = run.call("sample_outcomes", lev.sample_outcomes, "dice", inv, hor, seed=seed, device=dev, probs=probs)
    run.final("dice_sh_final_stats", "dice_sh_fixed_final_lev", lev.dice_sh_fixed_final_lev, dev, outcomes, top,
              VALUE_0, UP_R, DOWN_R, MID_R, SH_UP_R, SH_DOWN_R, SH_MID_R, l0_l, l0_h, l0_i)
    d, d_T = run.call("dice_sh_smart_lev", lev.dice_sh_smart_lev, dev, outcomes, inv, hor, top, VALUE_0, UP_R, DOWN_R,
                      MID_R, SH_UP_R, SH_DOWN_R, SH_MID_R, l1_l, l1_h, l1_i)
    run.save("dice_sh_inv1_val", d)
    run.save("dice_sh_inv1_val_T", d_T)
    run.total()
    return run.arrays


def gbm(INVESTORS=1e6, HORIZON=5e2, TOP=None, VALUE_0=1e2, drift=None, vol=None, name=None,
        l0_l=None, l0_h=None, l0_i=None, l1_l=None, l1_h=None, l1_i=None,
        path_results="./results/multiverse/", seed=420, device="cuda:0", log=print, timings=None):
    """lev/gbm.py: investor 1 in each GBM environment (defaults: gbm_op, gbm_snp).
    Every environment draws the same normals (stream 0; the reference reseeds per
    environment) scaled by its own log-mean and volatility."""
    drift = [0.05, 0.0540025395205692] if drift is None else drift
    vol = [float(np.sqrt(0.2)), 0.1897916175617430] if vol is None else vol
    name = ["gbm_op", "gbm_snp"] if name is None else name
    l0_l, l0_h, l0_i = ([-1.0, 0.4] if l0_l is None else l0_l, [1.0, 4.0] if l0_h is None else l0_h,
                        [0.2, 0.4] if l0_i is None else l0_i)
    l1_l, l1_h, l1_i = ([-1.0, 0.2] if l1_l is None else l1_l, [1.0, 2.0] if l1_h is None else l1_h,
                        [0.2, 0.2] if l1_i is None else l1_i)
    TOP, top = _top(TOP, INVESTORS)
    config.lev_gbm_tests(INVESTORS, HORIZON, TOP, VALUE_0, drift, vol, name, path_results, l0_l, l0_h, l0_i, l1_l, l1_h,
                         l1_i, log=log)
    log("GBM Experiment Tests: Passed")
    inv, hor = int(INVESTORS), int(HORIZON)
    run = _Run(path_results, device, log, timings)
    dev = run.dev
    for x in range(len(drift)):
        outcomes = run.call(f"{name[x]} sample_outcomes", lev.sample_outcomes, "gbm", inv, hor, seed=seed, device=dev,
                            log_mean=drift[x] - vol[x] ** 2 / 2, vol=vol[x])
        run.final(name[x] + "_final_stats", f"{name[x]} gbm_fixed_final_lev", lev.gbm_fixed_final_lev, dev, outcomes,
                  top, VALUE_0, l0_l[x], l0_h[x], l0_i[x])
        d, d_T = run.call(f"{name[x]} gbm_smart_lev", lev.gbm_smart_lev, dev, outcomes, inv, hor, top, VALUE_0, l1_l[x],
                          l1_h[x], l1_i[x])
        run.save(name[x] + "_inv1_val", d)
        run.save(name[x] + "_inv1_val_T", d_T)
        del outcomes, d, d_T
        run.total()
        run.timings[f"{name[x]} total"] = run.timings.pop("total")
    return run.arrays


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m rlmd_amd.lev_experiments",
                                 description="Run one of the reference's leverage experiments on the device.")
    ap.add_argument("experiment", choices=EXPERIMENTS)
    ap.add_argument("--investors", type=float, default=None, help="number of investors (default: the script's 1e6)")
    ap.add_argument("--horizon", type=float, default=None, help="time steps (default: the script's)")
    ap.add_argument("--out", default="./results/multiverse/", help="directory of the .npy files, relative (./.../)")
    ap.add_argument("--seed", type=int, default=420)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timings", default=None, help="write each call's wall time (ms, device-synchronised) as JSON")
    return ap


def _count(x):
    return int(x) if float(x).is_integer() else x


def main(argv=None):
    a = build_parser().parse_args(argv)
    kw = {"path_results": a.out if a.out.endswith("/") else a.out + "/", "seed": a.seed, "device": a.device}
    if a.investors is not None:
        kw["INVESTORS"] = _count(a.investors)
    if a.horizon is not None:
        kw["HORIZON"] = _count(a.horizon)
    timings = {}
    {"coin_flip": coin_flip, "dice_roll": dice_roll, "dice_roll_sh": dice_roll_sh, "gbm": gbm}[a.experiment](
        timings=timings, **kw)
    if a.timings:
        with open(a.timings, "w") as f:
            json.dump({"experiment": a.experiment, "investors": kw.get("INVESTORS"), "horizon": kw.get("HORIZON"),
                       "calls_ms": timings}, f)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
