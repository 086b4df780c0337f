"""Batched command line: many chains in one GPU session (SURVEY.md §5 "Config / flags").

The reference drives one ``./mcmc i < dataset`` process per chain from ``script.py``
(script.py:25-67, mcmc.c:102-210); ``build/mcmc`` keeps that exact contract.  This entry runs the
whole job at once and writes the same ``Chains/chain_NN`` tree:

    python -m seriation_amd DATASET [--chains 100] [--burnin 1000] [--samples 1000] [--thin 10]
                                    [--seed-base S] [--devices 0,1] [--root .] [--select K]
                                    [--no-save] [--debug-check] [--rng mt|philox] [--manycd]
                                    [--marginals] [--relations] [--waic] [--loo] [--modes [--mode-threshold X]]
                                    [--central] [--ppc [--ppc-seed S] [--ppc-reps R]] [--occupancy]
                                    [--place FILE]

  --thin        sweeps per saved sample (the reference's mcmc_sample runs 10, mcmc.c:225)
  --seed-base   chain k gets seed S + k; omitted -> unique 1-byte urandom seeds like
                script.py:25-38 (at most 256 chains)
  --select K    after the run, the one-sigma selection of choose_chains (script.py:70-98) over
                the written exp_data.csv files; prints the chosen chain indices
  --marginals   with --select: the posterior marginals of the chosen chains (analysis.marginals_from_records
                over their chain_data.csv, mirrored chains oriented first) into Chains/marginals.csv, one line
                per record column: kind (a, b, pi), index, mean, mode, the 2.5 %, 50 % and 97.5 % quantiles and
                the count of out-of-range values
  --relations   with --select: the relations between the chosen chains' taxa (analysis.relations_from_records over
                their chain_data.csv, mirrored chains oriented first).  Chains/diversity.csv: per position the
                mean and the 2.5 %, 50 % and 97.5 % quantiles of the number of taxa alive; Chains/taxon_pairs.csv:
                per pair i < j the counts of samples in which i originates before j and j before i, i ends before
                j and j before i, i is over before j begins and j before i begins, and the two coexist
  --waic        with --select: WAIC and the pointwise fit of the chosen chains (analysis.waic_from_records over their
                chain_data.csv, shared rates or, with --manycd, per-taxon rates).  Chains/waic.csv: one row
                elpd_waic, se, p_waic, lppd, waic, n_high (cells with p_waic above 0.4), samples, cells;
                Chains/waic_sites.csv and Chains/waic_taxa.csv: each site's and each taxon's share of elpd_waic
  --loo         with --select: PSIS-LOO cross-validation of the chosen chains (analysis.loo_from_records over their
                chain_data.csv, shared rates or, with --manycd, per-taxon rates).  Chains/loo.csv: one row elpd_loo,
                se, p_loo, lppd, looic, the cells with Pareto k <= 0.5, <= 0.7, <= 1 and above, the tail length,
                samples, cells; Chains/loo_sites.csv and Chains/loo_taxa.csv: each site's and each taxon's share of
                elpd_loo; Chains/loo_cells.csv: site, taxon, x, pareto_k, elpd_loo, lppd of the cells with k > 0.7 --
                the occurrences, and absences, to recheck
  --ppc         with --select: posterior predictive checks of the chosen chains (analysis.ppc_from_records over their
                chain_data.csv, shared rates or, with --manycd, per-taxon rates): --ppc-reps R (default 1, at most 64)
                replicate matrices per saved sample, drawn with --ppc-seed S (default 0), against the data on five
                discrepancies (ones, span, gaps, f0: false zeros, f1: false ones).  Chains/ppc.csv: per discrepancy
                the mean total of the data and of the replicates, the p-value (gt + eq / 2) / pairs and its counts;
                Chains/ppc_taxa.csv: the same means and p per taxon and discrepancy; Chains/ppc_sites.csv: per site
                its number of taxa in the data, the replicates' mean and p
  --occupancy   with --select: cell occupancy and the error tallies of the chosen chains (analysis.occupancy_from_records
                over their chain_data.csv; no orientation pass: nothing depends on the flips).  A taxon is alive at a
                site in a sample when the site's sampled position lies inside the taxon's sampled range.
                Chains/occupancy_cells.csv: site, taxon, x, alive (the samples in which the cell is alive), p_alive;
                Chains/occupancy_sites.csv: per site the row sum of X, the mean and the 2.5 %, 50 % and 97.5 %
                quantiles of the taxa alive, of the false zeros (alive, x = 0) and of the false ones (not alive,
                x = 1), and the completeness (the expected share of the taxa alive at the site that were found);
                Chains/occupancy_taxa.csv: the same per taxon over the sites, without the completeness
  --place FILE  with --select: where the rows of FILE belong in the seriation (analysis.placement_from_records over the
                chosen chains' chain_data.csv, mirrored chains oriented first, shared rates or, with --manycd,
                per-taxon rates).  FILE is in the dataset's format: a header `Q M`, then Q rows of M tokens 0, 1 or ?
                (not assessed).  A position means "of the same age as whichever site sits there", not an insertion
                between two sites.  Chains/placement.csv: per query its log predictive density, the mean, the mode and
                the 2.5 %, 50 % and 97.5 % quantiles of its position, the run's site it most probably shares its age
                with and that probability; Chains/placement_positions.csv: query, position, p;
                Chains/placement_sites.csv: query, site, p
  --modes       which chains sampled the same order, over all chains of the run, before and independent of --select
                (analysis.agreement_from_records and chain_modes over their chain_data.csv).  Chains/chain_modes.csv:
                per chain its mode, its flip against the mode's first chain, whether it is the mode's medoid, the
                mode's size and its distance to the medoid; Chains/chain_distances.csv: per pair k < l the order
                distance and the distance to l's mirror image, and per chain (k, k) the distance to its own mirror
                image; prints "modes: <n> sizes: ...".  --mode-threshold X (default 0.1, a default only: see
                analysis.chain_modes): chains are linked when their distance is at most X of the largest possible
  --central     with --select: the central sampled state of the chosen chains (analysis.central_from_records over
                their chain_data.csv, mirrored chains oriented first): the saved record with the smallest sum of
                Kendall distances to all the chosen chains' records, ties broken by the L1 distance of the taxon
                limits -- one coherent order with its ranges.  Chains/central_order.csv: site, position;
                Chains/central_taxa.csv: taxon, a, b; Chains/central_loss.csv: per chosen chain its flip, its best
                row with that row's order loss and limit loss, the sum of the chain's order losses, and whether it
                holds the central row; prints "central: chain <id> row <t>"
  --no-save     sample without writing files; prints one JSON summary per chain
  --rng         mt: GSL MT19937 as the reference (default); philox: the opt-in counter-based
                Philox4x32-10 stream for sampling (statistically equivalent, not bit-equal)
  --debug-check mcmc_consistent on every chain after every mcmc_sample call (the reference's
                MCMCDEBUG build, mcmc.c:249-255); with --no-save
  --manycd      per-taxon c, d (mcmc_readmodel's manycd = 1, mcmc.c:777-786, 807-816)

Prints the wall time (seconds, 2 decimals) as script.py:67 does.  Exit status 1 when a chain
fails its closing consistency check (mcmc.c:199-204).
"""
import argparse
import json
import os
import sys
import time

from . import core, launcher


def write_marginals(ds, chains, root, device=0):
    """Chains/marginals.csv of the chosen chains: their chain_data.csv rows, oriented against the first chain,
    pooled into one marginal per record column."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    r = analysis.marginals_from_records(ds, rec, probs=analysis.PROBS, flips=_oriented(ds, rec, device), device=device)
    with open(os.path.join(root, "Chains", "marginals.csv"), "w") as fh:
        fh.write("kind,index,mean,mode,%s,outside\n" % ",".join("q%s" % p for p in analysis.PROBS))
        for kind in ("a", "b", "pi"):
            for j in range(len(r["mode"][kind])):
                fh.write("%s,%d,%r,%d,%s,%d\n" % (kind, j, float(r["mean"][kind][j]), r["mode"][kind][j],
                                                  ",".join(str(q) for q in r["quant"][kind][:, j]),
                                                  r["outside"][kind][j]))


def _oriented(ds, rec, device):
    """the chains' flips against the first chain, as write_marginals takes them"""
    from . import analysis
    return analysis.chain_orientation(analysis.marginals_from_records(ds, rec, probs=(), device=device)["pi_sum"])


def write_relations(ds, chains, root, device=0):
    """Chains/diversity.csv and Chains/taxon_pairs.csv of the chosen chains: their chain_data.csv rows, oriented
    against the first chain, pooled into exact counts."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    r = analysis.relations_from_records(ds, rec, flips=_oriented(ds, rec, device), device=device)
    dc = analysis.diversity_curve(r["rich_hist"], analysis.PROBS)
    with open(os.path.join(root, "Chains", "diversity.csv"), "w") as fh:
        fh.write("position,mean,%s\n" % ",".join("q%s" % p for p in analysis.PROBS))
        for p in range(ds.N):
            fh.write("%d,%r,%s\n" % (p, float(dc["mean"][p]), ",".join(str(q) for q in dc["quant"][:, p])))
    ob, eb, pr, ov = (r[k].tolist() for k in ("orig_before", "ext_before", "precedes", "overlap"))
    with open(os.path.join(root, "Chains", "taxon_pairs.csv"), "w") as fh:
        fh.write("i,j,orig_ij,orig_ji,ext_ij,ext_ji,prec_ij,prec_ji,overlap\n")
        for i in range(ds.M):
            for j in range(i + 1, ds.M):
                fh.write("%d,%d,%d,%d,%d,%d,%d,%d,%d\n" % (i, j, ob[i][j], ob[j][i], eb[i][j], eb[j][i], pr[i][j],
                                                          pr[j][i], ov[i][j]))


def write_occupancy(ds, chains, root, device=0):
    """Chains/occupancy_cells.csv, Chains/occupancy_sites.csv and Chains/occupancy_taxa.csv of the chosen chains: the
    exact occupancy counts over their chain_data.csv rows."""
    import numpy as np
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    r = analysis.occupancy_from_records(ds, rec, device=device)
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M).astype(bool)
    alive, p = r["alive"].tolist(), r["p_alive"].tolist()
    with open(os.path.join(root, "Chains", "occupancy_cells.csv"), "w") as fh:
        fh.write("site,taxon,x,alive,p_alive\n")
        for n in range(ds.N):
            for m in range(ds.M):
                fh.write("%d,%d,%d,%d,%r\n" % (n, m, X[n, m], alive[n][m], p[n][m]))
    cols = ",".join("%s_mean,%s" % (k, ",".join("%s_q%s" % (k, q) for q in analysis.PROBS))
                    for k in ("alive", "f0", "f1"))

    def bands(prefix, j):
        out = []
        for k in ("alive", "f0", "f1"):
            dc = curves[prefix + k]
            out.append("%r,%s" % (float(dc["mean"][j]), ",".join(str(q) for q in dc["quant"][:, j])))
        return ",".join(out)

    curves = {k[:-5]: analysis.diversity_curve(r[k], analysis.PROBS) for k in analysis.OCC_KINDS if k != "alive"}
    with open(os.path.join(root, "Chains", "occupancy_sites.csv"), "w") as fh:
        fh.write("site,x_sum,%s,completeness\n" % cols)
        for n in range(ds.N):
            fh.write("%d,%d,%s,%r\n" % (n, X[n].sum(), bands("site_", n), float(r["site_completeness"][n])))
    with open(os.path.join(root, "Chains", "occupancy_taxa.csv"), "w") as fh:
        fh.write("taxon,x_sum,%s\n" % cols)
        for m in range(ds.M):
            fh.write("%d,%d,%s\n" % (m, X[:, m].sum(), bands("taxon_", m)))


def write_placement(ds, chains, root, queries, manycd=False, device=0):
    """Chains/placement.csv, Chains/placement_positions.csv and Chains/placement_sites.csv of the chosen chains: the
    placement of the query rows [Q][M] over their chain_data.csv rows, oriented against the first chain, the rates
    read back from the files' c and d tokens."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    cd = analysis.read_chain_cd(root, chains, ds.M, manycd=manycd)
    r = analysis.placement_from_records(ds, rec, cd, queries, manycd=manycd, flips=_oriented(ds, rec, device),
                                        device=device)
    s = analysis.placement_summary(r["pos"], r["site"], analysis.PROBS)
    Q = r["pos"].shape[0]
    with open(os.path.join(root, "Chains", "placement.csv"), "w") as fh:
        fh.write("query,lpd,mean,mode,%s,best_site,p_best_site\n" % ",".join("q%s" % p for p in analysis.PROBS))
        for q in range(Q):
            fh.write("%d,%r,%r,%d,%s,%d,%r\n" % (q, float(r["lpd"][q]), float(s["mean"][q]), s["mode"][q],
                                                 ",".join(str(v) for v in s["quant"][:, q]), s["best_site"][q],
                                                 float(s["p_best_site"][q])))
    for name, key, col in (("placement_positions.csv", "pos", "position"), ("placement_sites.csv", "site", "site")):
        v = r[key].tolist()
        with open(os.path.join(root, "Chains", name), "w") as fh:
            fh.write("query,%s,p\n" % col)
            for q in range(Q):
                for j in range(ds.N):
                    fh.write("%d,%d,%r\n" % (q, j, v[q][j]))


def write_ppc(ds, chains, root, manycd=False, seed=0, reps=1, device=0):
    """Chains/ppc.csv, Chains/ppc_taxa.csv and Chains/ppc_sites.csv of the chosen chains: posterior predictive checks
    over their chain_data.csv rows, the rates read back from the files' c and d tokens."""
    import numpy as np
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    cd = analysis.read_chain_cd(root, chains, ds.M, manycd=manycd)
    r = analysis.ppc_from_records(ds, rec, cd, manycd=manycd, seed=seed, reps=reps, device=device)
    pairs = float(r["pairs"])
    with open(os.path.join(root, "Chains", "ppc.csv"), "w") as fh:
        fh.write("stat,obs_mean,rep_mean,p,gt,eq,pairs\n")
        for i, name in enumerate(analysis.PPC_STATS):
            fh.write("%s,%r,%r,%r,%d,%d,%d\n" % (name, float(int(r["taxon_sum_obs"][i].sum())) / pairs,
                                                 float(int(r["taxon_sum_rep"][i].sum())) / pairs,
                                                 float(r["p_total"][i]), r["total_gt"][i], r["total_eq"][i],
                                                 r["pairs"]))
    with open(os.path.join(root, "Chains", "ppc_taxa.csv"), "w") as fh:
        fh.write("taxon,stat,obs_mean,rep_mean,p\n")
        for m in range(ds.M):
            for i, name in enumerate(analysis.PPC_STATS):
                fh.write("%d,%s,%r,%r,%r\n" % (m, name, float(r["taxon_sum_obs"][i, m]) / pairs,
                                               float(r["taxon_sum_rep"][i, m]) / pairs, float(r["p_taxon"][i, m])))
    obs = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M).astype(bool).sum(axis=1)
    with open(os.path.join(root, "Chains", "ppc_sites.csv"), "w") as fh:
        fh.write("site,obs,rep_mean,p\n")
        for n in range(ds.N):
            fh.write("%d,%d,%r,%r\n" % (n, obs[n], float(r["site_sum_rep"][n]) / pairs, float(r["p_site"][n])))


def write_waic(ds, chains, root, manycd=False, device=0):
    """Chains/waic.csv, Chains/waic_sites.csv and Chains/waic_taxa.csv of the chosen chains: WAIC over their
    chain_data.csv rows, the rates read back from the files' c and d tokens."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    cd = analysis.read_chain_cd(root, chains, ds.M, manycd=manycd)
    r = analysis.waic_from_records(ds, rec, cd, manycd=manycd, pointwise=False, device=device)
    with open(os.path.join(root, "Chains", "waic.csv"), "w") as fh:
        fh.write("elpd_waic,se,p_waic,lppd,waic,n_high,samples,cells\n")
        fh.write("%r,%r,%r,%r,%r,%d,%d,%d\n" % (float(r["elpd_waic"]), float(r["se"]), float(r["p_waic"]),
                                                float(r["lppd_sum"]), float(r["waic"]), r["n_high"], r["total"],
                                                ds.N * ds.M))
    for name, key, n in (("waic_sites.csv", "site", ds.N), ("waic_taxa.csv", "taxon", ds.M)):
        with open(os.path.join(root, "Chains", name), "w") as fh:
            fh.write("%s,elpd\n" % key)
            for i in range(n):
                fh.write("%d,%r\n" % (i, float(r[key + "_elpd"][i])))


def write_loo(ds, chains, root, manycd=False, device=0):
    """Chains/loo.csv, Chains/loo_sites.csv, Chains/loo_taxa.csv and Chains/loo_cells.csv of the chosen chains:
    PSIS-LOO over their chain_data.csv rows, the rates read back from the files' c and d tokens."""
    import numpy as np
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    cd = analysis.read_chain_cd(root, chains, ds.M, manycd=manycd)
    r = analysis.loo_from_records(ds, rec, cd, manycd=manycd, device=device)
    with open(os.path.join(root, "Chains", "loo.csv"), "w") as fh:
        fh.write("elpd_loo,se,p_loo,lppd,looic,k_le_0.5,k_le_0.7,k_le_1,k_gt_1,tail,samples,cells\n")
        fh.write("%r,%r,%r,%r,%r,%d,%d,%d,%d,%d,%d,%d\n" % (
            (float(r["elpd_loo"]), float(r["se"]), float(r["p_loo"]), float(r["lppd_sum"]), float(r["looic"]))
            + tuple(r["n_k"]) + (r["tail_len"], r["total"], ds.N * ds.M)))
    for name, key, n in (("loo_sites.csv", "site", ds.N), ("loo_taxa.csv", "taxon", ds.M)):
        with open(os.path.join(root, "Chains", name), "w") as fh:
            fh.write("%s,elpd\n" % key)
            for i in range(n):
                fh.write("%d,%r\n" % (i, float(r[key + "_elpd"][i])))
    X = np.ctypeslib.as_array(ds.c.X, (ds.N * ds.M,)).reshape(ds.N, ds.M)
    with open(os.path.join(root, "Chains", "loo_cells.csv"), "w") as fh:
        fh.write("site,taxon,x,pareto_k,elpd_loo,lppd\n")
        for n, m in zip(*np.nonzero(r["pareto_k"] > 0.7)):
            fh.write("%d,%d,%d,%r,%r,%r\n" % (n, m, X[n, m] != 0, float(r["pareto_k"][n, m]), float(r["elpd"][n, m]),
                                              float(r["lppd"][n, m])))


def write_modes(ds, chains, root, threshold, device=0):
    """Chains/chain_modes.csv and Chains/chain_distances.csv of all the run's chains: the order distances between
    their chain_data.csv rows and the modes linked at `threshold`.  Returns the modes' sizes."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    r = analysis.agreement_from_records(ds, rec, device=device)
    d, dm = r["dist"].tolist(), r["dist_mirror"].tolist()
    cm = analysis.chain_modes(r["dist"], r["dist_mirror"], r["scale"], threshold)
    n = len(chains)
    with open(os.path.join(root, "Chains", "chain_modes.csv"), "w") as fh:
        fh.write("chain,mode,flip,is_medoid,mode_size,dist_to_medoid\n")
        for k in range(n):
            g = int(cm["mode"][k])
            c = int(cm["medoid"][g])
            lo, hi = min(k, c), max(k, c)
            fh.write("%d,%d,%d,%d,%d,%d\n" % (chains[k], g, cm["flip"][k], k == c, cm["size"][g],
                                              0 if k == c else min(d[lo][hi], dm[lo][hi])))
    with open(os.path.join(root, "Chains", "chain_distances.csv"), "w") as fh:
        fh.write("k,l,dist,dist_mirror\n")
        for k in range(n):
            fh.write("%d,%d,%d,%d\n" % (chains[k], chains[k], d[k][k], dm[k][k]))
            for l in range(k + 1, n):
                fh.write("%d,%d,%d,%d\n" % (chains[k], chains[l], d[k][l], dm[k][l]))
    return cm["size"].tolist()


def write_central(ds, chains, root, device=0):
    """Chains/central_order.csv, Chains/central_taxa.csv and Chains/central_loss.csv of the chosen chains: their
    chain_data.csv rows, oriented against the first chain, and the row of smallest expected loss among them.  Returns
    (chain id, row) of that row."""
    from . import analysis
    rec = analysis.read_chain_rows(root, chains, ds.N, ds.M)
    flips = _oriented(ds, rec, device)
    r = analysis.central_from_records(ds, rec, flips=flips, device=device)
    ck, ct = r["central"]
    with open(os.path.join(root, "Chains", "central_order.csv"), "w") as fh:
        fh.write("site,position\n")
        for n in range(ds.N):
            fh.write("%d,%d\n" % (n, r["state"]["pi"][n]))
    with open(os.path.join(root, "Chains", "central_taxa.csv"), "w") as fh:
        fh.write("taxon,a,b\n")
        for m in range(ds.M):
            fh.write("%d,%d,%d\n" % (m, r["state"]["a"][m], r["state"]["b"][m]))
    ol, ll = r["order_loss"].tolist(), r["limit_loss"].tolist()
    with open(os.path.join(root, "Chains", "central_loss.csv"), "w") as fh:
        fh.write("chain,flip,best_row,order_loss,limit_loss,order_loss_sum,is_central\n")
        for k in range(len(chains)):
            t = int(r["best"][k])
            fh.write("%d,%d,%d,%d,%d,%d,%d\n" % (chains[k], flips[k], t, ol[k][t], ll[k][t], sum(ol[k]), k == ck))
    return chains[ck], ct


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seriation_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("dataset")
    ap.add_argument("--chains", type=int, default=100)
    ap.add_argument("--burnin", type=int, default=1000, help="burn-in mcmc_sample calls")
    ap.add_argument("--samples", type=int, default=1000, help="saved mcmc_sample calls")
    ap.add_argument("--thin", type=int, default=10, help="sweeps per mcmc_sample call")
    ap.add_argument("--seed-base", type=int, default=None)
    ap.add_argument("--devices", default="0", help="comma-separated GPU ordinals")
    ap.add_argument("--root", default=".")
    ap.add_argument("--select", type=int, default=0)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--debug-check", action="store_true")
    ap.add_argument("--rng", default="mt", choices=("mt", "philox"))
    ap.add_argument("--manycd", action="store_true")
    ap.add_argument("--marginals", action="store_true")
    ap.add_argument("--relations", action="store_true")
    ap.add_argument("--waic", action="store_true")
    ap.add_argument("--loo", action="store_true")
    ap.add_argument("--ppc", action="store_true")
    ap.add_argument("--ppc-seed", type=int, default=0)
    ap.add_argument("--ppc-reps", type=int, default=1)
    ap.add_argument("--occupancy", action="store_true")
    ap.add_argument("--place", default=None, metavar="FILE")
    ap.add_argument("--modes", action="store_true")
    ap.add_argument("--mode-threshold", type=float, default=0.1)
    ap.add_argument("--central", action="store_true")
    a = ap.parse_args(argv)
    if a.modes and a.no_save:
        ap.error("--modes needs the chain files: not with --no-save")
    if a.modes and not 0.0 <= a.mode_threshold <= 1.0:
        ap.error("--mode-threshold must lie in [0, 1]")
    if a.waic and (a.select < 1 or a.no_save):
        ap.error("--waic needs --select K (and the chain files: not with --no-save)")
    if a.loo and (a.select < 1 or a.no_save):
        ap.error("--loo needs --select K (and the chain files: not with --no-save)")
    if a.ppc and (a.select < 1 or a.no_save):
        ap.error("--ppc needs --select K (and the chain files: not with --no-save)")
    if a.ppc and not (1 <= a.ppc_reps <= 64 and 0 <= a.ppc_seed < 2 ** 64):
        ap.error("--ppc-reps must lie in 1..64 and --ppc-seed in 0..2^64-1")
    if a.occupancy and (a.select < 1 or a.no_save):
        ap.error("--occupancy needs --select K (and the chain files: not with --no-save)")
    if a.place and (a.select < 1 or a.no_save):
        ap.error("--place needs --select K (and the chain files: not with --no-save)")
    if a.marginals and (a.select < 1 or a.no_save):
        ap.error("--marginals needs --select K (and the chain files: not with --no-save)")
    if a.relations and (a.select < 1 or a.no_save):
        ap.error("--relations needs --select K (and the chain files: not with --no-save)")
    if a.central and (a.select < 1 or a.no_save):
        ap.error("--central needs --select K (and the chain files: not with --no-save)")
    if a.chains < 1 or a.burnin < 0 or a.samples < 0 or a.thin < 1:
        ap.error("--chains and --thin must be >= 1, --burnin and --samples >= 0")
    devices = [int(d) for d in a.devices.split(",") if d.strip()]
    if a.seed_base is None:
        if a.chains > 256:
            ap.error("urandom 1-byte seeds (script.py:25-38) allow at most 256 chains; pass --seed-base")
        old = []
        seeds = [launcher._unique_seed(old) for _ in range(a.chains)]
    else:
        seeds = [a.seed_base + k for k in range(a.chains)]
    if a.debug_check and not a.no_save:
        ap.error("--debug-check runs with --no-save")
    if a.no_save:
        ds = core.Dataset.load(a.dataset)
        t0 = time.perf_counter()
        summ, _ = core.run_chains(ds, seeds, burnin_calls=a.burnin, sample_calls=a.samples,
                                  sweeps_per_call=a.thin, devices=devices[:len(seeds)], debug_check=a.debug_check,
                                  rng=a.rng, manycd=int(a.manycd))
        wall = time.perf_counter() - t0
        for s in summ:
            print(json.dumps(s))
        print(round(wall, 2))
    else:
        summ = launcher.run_all_chains(a.dataset, n_chains=a.chains, seeds=seeds, devices=devices,
                                       burnin_calls=a.burnin, sample_calls=a.samples, root=a.root,
                                       sweeps_per_call=a.thin, rng=a.rng, manycd=int(a.manycd))
        if a.modes:
            sizes = write_modes(core.Dataset.load(a.dataset), list(range(a.chains)), a.root, a.mode_threshold,
                                devices[0] if devices else 0)
            print("modes: %d sizes: %s" % (len(sizes), " ".join(str(v) for v in sizes)))
        if a.select:
            chosen = launcher.choose_chains(a.select, a.root)
            print("selected:", " ".join(str(k) for k in chosen))
            if a.marginals:
                write_marginals(core.Dataset.load(a.dataset), chosen, a.root, devices[0] if devices else 0)
            if a.relations:
                write_relations(core.Dataset.load(a.dataset), chosen, a.root, devices[0] if devices else 0)
            if a.waic:
                write_waic(core.Dataset.load(a.dataset), chosen, a.root, a.manycd, devices[0] if devices else 0)
            if a.loo:
                write_loo(core.Dataset.load(a.dataset), chosen, a.root, a.manycd, devices[0] if devices else 0)
            if a.ppc:
                write_ppc(core.Dataset.load(a.dataset), chosen, a.root, a.manycd, a.ppc_seed, a.ppc_reps,
                          devices[0] if devices else 0)
            if a.occupancy:
                write_occupancy(core.Dataset.load(a.dataset), chosen, a.root, devices[0] if devices else 0)
            if a.place:
                ds = core.Dataset.load(a.dataset)
                from . import analysis
                write_placement(ds, chosen, a.root, analysis.read_queries(a.place, ds.M), a.manycd,
                                devices[0] if devices else 0)
            if a.central:
                print("central: chain %d row %d" % write_central(core.Dataset.load(a.dataset), chosen, a.root,
                                                                  devices[0] if devices else 0))
    return 1 if any(s.get("consistent", 0) for s in summ) else 0


if __name__ == "__main__":
    sys.exit(main())
