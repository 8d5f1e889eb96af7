"""hot_path_batch: steps 4 (site calling) to 11 of the pipeline as ONE job — every pileup crosses the host link once.

Once while the rank's pileups fit the resident budget (route ``resident``: they are kept in HBM between site calling and the
consensus scan), and once at ANY size where the device does not write var.flt.vcf (``--siteCalling existing`` / ``varscan``, route
``stream``: both site lists are known before the first pileup byte moves, so the consensus stage scans and calls each file as it
lands and nothing is kept).  ``--pileupRoute auto`` (the default) takes ``stream`` exactly where ``resident`` would have to read
files a second time; mode ``device`` past the budget still reads those files twice (its site calling needs the file first).

The reference runs these steps as separate process arrays over a shared file system (run.py:662-784): call_sites
(call_sites.py:89-108), filter_regions, merge_sites twice, call_consensus twice per sample (run.py:704-710 and :712-718),
snp_matrix twice, snp_reference twice, distance twice — and every one of call_sites and the two call_consensus passes reads the
sample's reads.all.pileup (0.4 GB per 5 Mbp x 30x sample) again.  This module is the same chain of steps, writing the same
files with the same bytes, arranged around the device instead of around the file system.  The job is a sequence of STAGES over
one explicit state object (``_Job``); a stage is a plain function of the job and can be driven alone:

  stage_ingest_and_sites      every rank (= one GPU; torchrun-able) streams the pileups of ITS samples (a contiguous block of
                              the sorted sample directories) into HBM and KEEPS them (``Device.pileups``; files past the memory
                              budget are re-streamed by the consensus stage; on route ``stream`` nothing is copied here: the
                              pileups are only opened, so that an unreadable one fails its sample before the site union, as the
                              ingest would have).  Where var.flt.vcf comes from is the site calling
                              mode (``--siteCalling``, call_sites.py): ``device`` — site calling (csrc/varscan.hip) runs on each
                              file while the next one arrives and host threads finish each sample as its records come back;
                              ``varscan`` — the VarScan jar, as the reference runs it, on host threads beside the ingest;
                              ``existing`` — the files are inputs and are never written
  stage_site_union_and_regions  C1: all-gather of every sample's (CHROM, POS) records; dense-region filter (K3), both site unions
                              (K4) on every rank — identical results everywhere; rank 0 writes snplist.txt / snplist_preserved.txt
                              and the two filtered directory lists, every rank the var.flt_preserved.vcf / var.flt_removed.vcf of
                              its samples
  stage_consensus             ONE scan + call over the resident pileups at the positions of snplist.txt, with per-site records
                              (route ``stream``: one streamed call per group of samples that leaves the same rows on the device,
                              ``Device.call_consensus_files_dev``);
                              the preserved flow (snplist_preserved.txt columns, ``Region`` for the sample's removed positions) is
                              derived from it on the device (csrc/flows.hip); consensus.fasta / consensus.vcf /
                              consensus_preserved.fasta / consensus_preserved.vcf of a group of samples are written by host threads
                              while the next group is on the device
  stage_matrices_and_distances  4-bit pack of both matrices, C2 all-gather of the rows, all-pairs distance tiles dealt to the
                              ranks, row-band exchange; snpma*.fasta (every rank writes its block of the file), the four TSVs and
                              referenceSNP*.fasta (rank 0)
  stage_leftover_vcfs         the VCF files the per-sample command has to write (repeated positions, --vcfAllPos)

Between stages the ranks AGREE on failure (``_Job.agree``): a rank whose stage raised does not leave its peers waiting in the
next collective — every rank learns of it, the failing rank reports its own error, all leave with the same exit code.  Inside a
stage, collectives come first and rank-local work that can fail (file output) after them, or under ``_Job.guard``.

Options of the individual steps are given as the reference gives them: the ``*_ExtraParams`` strings (argument or the
environment variable of the same name), parsed by the step's own argument parser.
"""
from __future__ import print_function

import argparse
import concurrent.futures
import contextlib
import ctypes
import datetime
import os
import shlex
import sys
import threading
import time

import numpy as np

from . import _lib as L
from . import call_sites as cs
from . import device as devmod
from . import distance as dmod
from . import filter_regions as fr
from . import merge_sites as ms
from . import snp_reference
from . import utils
from . import varscan
from . import vcf_writer
from .utils import verbose_print

INGEST_BATCH = 128          # files per streamed ingest call (the record arrays of a call are files x capacity x 48 bytes)
VARSCAN_CAPACITY = 16384    # records per file in those arrays; a file with more is repeated alone


PILEUP_ROUTES = ("resident", "stream", "auto")
STREAM_MODES = ("existing", "varscan")      # site calling modes in which the device never looks at a pileup before the site lists exist


def pileup_route_setting(given=None):
    """`given` (a --pileupRoute option) or $SNPGPU_PILEUP_ROUTE or auto."""
    route = (given or os.environ.get("SNPGPU_PILEUP_ROUTE") or "auto").lower()
    if route not in PILEUP_ROUTES:
        utils.global_error("Error: pileup route must be one of %s, not %r." % (", ".join(PILEUP_ROUTES), route))
    return route


def resolve_pileup_route(setting, site_calling, rank_bytes, budget_bytes):
    """resident or stream for one rank.  ``auto`` is ``stream`` where the site lists do not need the device (STREAM_MODES) AND the
    rank's pileup bytes exceed the resident budget — where the resident route would stream files a second time; every job that
    fits keeps the resident route.  (An explicit ``stream`` in mode ``device`` is refused by the job, not here.)"""
    if setting == "auto":
        return "stream" if site_calling in STREAM_MODES and int(rank_bytes) > int(budget_bytes) else "resident"
    return setting


class _Sample(object):
    __slots__ = ("index", "dir", "name", "pileup", "ok", "error", "store_index", "vcf_lines", "header", "sites", "removed",
                 "n_lines", "n_rows", "names_escaped")

    def __init__(self, index, sample_dir, pileup_name):
        self.index = index                      # position in the sorted list of sample directories
        self.dir = sample_dir
        self.name = os.path.basename(os.path.abspath(sample_dir))   # basename(dirname(<dir>/file)), as every step derives it
        self.pileup = os.path.join(sample_dir, pileup_name)
        self.ok = True
        self.error = None
        self.store_index = -1
        self.vcf_lines = self.header = self.sites = self.removed = None
        self.n_lines = self.n_rows = 0
        self.names_escaped = False              # its pileup spells contig names that are not plain ASCII: the device reads an escaped copy

    def fail(self, message):
        self.ok, self.error = False, message


def _step_args(step, fixed, extra):
    """The Namespace the step's own parser makes of its ExtraParams string (flags, defaults and validators are the CLI's)."""
    from . import cfsan_snp_pipeline as cli
    return cli.parse_argument_list([step] + shlex.split(extra or "") + fixed)


class _Comm(object):
    """torch.distributed when the job has more than one rank (backend nccl = RCCL over xGMI; gloo in the one-GPU tests)."""

    def __init__(self):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.one_gpu = os.environ.get("SNPGPU_PIPELINE_ONE_GPU") == "1"      # functional tests: all ranks on device 0 over gloo
        self.dist = None
        self.owns_group = False
        if self.one_gpu:
            self.local_rank = 0
        if self.world > 1 or os.environ.get("SNPGPU_DIST_AT_WORLD_1") == "1":      # (the second: sharding.group_of_one_exchanges, tests)
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(self.local_rank)
            if not dist.is_initialized():
                if self.one_gpu:
                    dist.init_process_group("gloo")
                else:
                    dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))
                self.owns_group = True
            self.dist = dist

    def close(self):
        """Leave the process group this job created (its helper threads must not outlive the interpreter's teardown)."""
        if self.dist and self.owns_group and self.dist.is_initialized():
            self.dist.destroy_process_group()
            self.owns_group = False

    def barrier(self):
        if self.dist:
            import torch
            torch.cuda.synchronize()
            self.dist.barrier()

    def gather_objects(self, obj):
        """[obj of rank 0, obj of rank 1, ...] on every rank (small things only: names, sizes, error counts)."""
        if not self.dist:
            return [obj]
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out


class _Job(object):
    """Everything the stages of one hot_path_batch job share.  Set up by ``_Job.__init__`` (arguments, samples, the rank's
    shard, device + resident store); each stage documents the fields it adds."""

    def __init__(self, args, comm):
        import torch                                   # device tensors, pinned host buffers and the collectives: plumbing
        from . import sharding
        self.torch, self.sharding = torch, sharding
        self.args, self.comm = args, comm
        self.rank, self.world = comm.rank, comm.world
        self.t_start = time.perf_counter()
        self.timings = {}
        self.call_passes = {}                          # lines each call kernel took, summed over the groups (Device.call_pass_counts)
        self.deferred = None                           # first exception of a guarded block (see guard)
        self.dev = self.store = None

        # ---- arguments: what run.py:662-784 puts on the command lines of the steps ---------------------------------------
        self.dirs_file = dirs_file = args.sampleDirsFile
        self.ref_path = ref_path = args.referenceFile
        if utils.verify_non_empty_input_files("File of sample directories", [dirs_file]) > 0:
            utils.global_error(None)
        utils.verify_non_empty_input_files("Reference file", [ref_path], error_handler="global")
        with open(dirs_file, "r") as f:
            self.unsorted_dirs = [d for d in (line.rstrip() for line in f) if d]
        self.sorted_dirs = sorted(self.unsorted_dirs)
        self.dir_index = {d: i for i, d in enumerate(self.sorted_dirs)}
        self.work_dir = work_dir = args.workDir or os.path.dirname(os.path.abspath(dirs_file))

        def env(name, given):
            return given if given is not None else (os.environ.get(name) or "")

        self.fr_args = _step_args("filter_regions", ["-n", "var.flt.vcf", dirs_file, ref_path], env("FilterRegions_ExtraParams", args.filterRegionsExtraParams))
        self.ms_args = _step_args("merge_sites", [dirs_file, dirs_file + ".OrigVCF.filtered"], env("MergeSites_ExtraParams", args.mergeSitesExtraParams))
        self.cc_extra = env("CallConsensus_ExtraParams", args.callConsensusExtraParams)
        self.cc_args = _step_args("call_consensus", ["--vcfRefName", os.path.basename(ref_path), "--vcfFileName", "consensus.vcf", "x.pileup"], self.cc_extra)
        self.vs_opts = varscan.Options(env("VarscanMpileup2snp_ExtraParams", args.varscanExtraParams))
        self.site_calling = cs.site_calling_mode(getattr(args, "siteCalling", None))
        self.route_setting = pileup_route_setting(getattr(args, "pileupRoute", None))
        if self.route_setting == "stream" and self.site_calling not in STREAM_MODES:
            utils.global_error("Error: --pileupRoute stream needs the site lists before the first pileup is read, so it goes with --siteCalling existing "
                               "or varscan only: in mode %s the device calls the sites of each pileup, and that needs the file first." % self.site_calling)
        self.pileup_route = None                       # resident / stream: resolved when the device is open (open_device)
        self.want_vcf = not args.noConsensusVcf
        # --collectMetrics: the metrics files (and the table) at the end of the job, from what the job holds (stage_collect_metrics)
        self.collect_metrics = bool(getattr(args, "collectMetrics", False))
        self.cm_extra = env("CollectMetrics_ExtraParams", getattr(args, "collectMetricsExtraParams", None))
        self.metrics_known = {}                        # sample dir -> {"depth_sum", "missingPos", "missingPosPreserved"}
        # --vcfAllPos (a row for every line of the pileup, call_consensus.py:148-151) is the per-sample command's all-lines pass: the
        # job writes the FASTA files and everything downstream, and lets that command write every sample's two VCF files at the end
        self.vcf_all_pos = bool(self.cc_args.vcfAllPos and self.want_vcf)
        if self.vcf_all_pos:
            self.want_vcf = False
        self.outputs = {k: os.path.join(work_dir, v) for k, v in (
            ("snplist", "snplist.txt"), ("snplist_p", "snplist_preserved.txt"), ("snpma", "snpma.fasta"), ("snpma_p", "snpma_preserved.fasta"),
            ("pairs", "snp_distance_pairwise.tsv"), ("matrix", "snp_distance_matrix.tsv"), ("pairs_p", "snp_distance_pairwise_preserved.tsv"),
            ("matrix_p", "snp_distance_matrix_preserved.tsv"), ("refsnp", "referenceSNP.fasta"), ("refsnp_p", "referenceSNP_preserved.fasta"))}
        # --closePairs / --clusters (additive to the distance step): the pairwise rows within a distance, single-linkage groups
        self.close_pairs = getattr(args, "closePairs", None)
        self.cluster_thresholds = dmod.cluster_thresholds(getattr(args, "clusters", None) or [])
        if (self.close_pairs is not None and self.close_pairs < 0) or any(t < 0 for t in self.cluster_thresholds):
            utils.global_error("Error: a distance threshold cannot be negative.")
        if self.close_pairs is not None:
            self.outputs.update(close=os.path.join(work_dir, "snp_distance_close_pairs.tsv"), close_p=os.path.join(work_dir, "snp_distance_close_pairs_preserved.tsv"))
        if self.cluster_thresholds:
            self.outputs.update(clusters=os.path.join(work_dir, "snp_clusters.tsv"), clusters_p=os.path.join(work_dir, "snp_clusters_preserved.tsv"))
        # --mst (additive to the distance step): the minimum spanning tree of the samples and their single-linkage dendrogram
        self.mst = bool(getattr(args, "mst", False))
        if self.mst:
            self.outputs.update(mst=os.path.join(work_dir, "snp_mst.tsv"), mst_p=os.path.join(work_dir, "snp_mst_preserved.tsv"),
                                dendrogram=os.path.join(work_dir, "snp_dendrogram.nwk"), dendrogram_p=os.path.join(work_dir, "snp_dendrogram_preserved.nwk"))
        # --linkage (additive to the distance step): the complete- or average-linkage tree, its dendrogram and, with --clusters, its cuts
        self.linkage = getattr(args, "linkage", None)
        if self.linkage:
            self.outputs.update(linkage=os.path.join(work_dir, "snp_linkage.tsv"), linkage_p=os.path.join(work_dir, "snp_linkage_preserved.tsv"),
                                linkage_nwk=os.path.join(work_dir, "snp_linkage.nwk"), linkage_nwk_p=os.path.join(work_dir, "snp_linkage_preserved.nwk"))
            if self.cluster_thresholds:
                self.outputs.update(linkage_clusters=os.path.join(work_dir, "snp_linkage_clusters.tsv"),
                                    linkage_clusters_p=os.path.join(work_dir, "snp_linkage_clusters_preserved.tsv"))
        # --nj (additive to the distance step): the neighbour-joining tree as a Newick line
        self.nj = bool(getattr(args, "nj", False))
        if self.nj:
            self.outputs.update(nj=os.path.join(work_dir, "snp_nj.nwk"), nj_p=os.path.join(work_dir, "snp_nj_preserved.nwk"))
        # --pairSites (additive to the distance step): the sites at which the close pairs / the tree's edges differ
        self.pair_sites = bool(getattr(args, "pairSites", False))
        if self.pair_sites and self.close_pairs is None and not self.mst:
            utils.global_error("Error: --pairSites needs --closePairs or --mst.")
        if self.pair_sites and self.close_pairs is not None:
            self.outputs.update(close_sites=os.path.join(work_dir, "snp_close_pair_sites.tsv"), close_sites_p=os.path.join(work_dir, "snp_close_pair_sites_preserved.tsv"))
        if self.pair_sites and self.mst:
            self.outputs.update(mst_sites=os.path.join(work_dir, "snp_mst_sites.tsv"), mst_sites_p=os.path.join(work_dir, "snp_mst_sites_preserved.tsv"))
        self.filtered1, self.filtered2 = dirs_file + ".OrigVCF.filtered", dirs_file + ".PresVCF.filtered"

        self.samples = [_Sample(i, d, args.pileupName) for i, d in enumerate(self.sorted_dirs)]
        self.n_total = len(self.samples)
        self.lo, self.hi = sharding.shard_bounds(self.n_total, self.rank, self.world)
        self.mine = self.samples[self.lo:self.hi]
        self.group_bytes = int(args.groupBytes) if args.groupBytes else (1 << 30)
        self.arenas = [None, None]
        self.arena_thread = None
        self.h2d_extra = 0
        self.stream_stats = {"file_bytes": 0, "files": 0, "seconds": 0.0, "readers": 0}      # route stream: summed over the group calls

    # ---- small services of the state object ----------------------------------------------------------------------------------
    def lap(self, name, t0):
        self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0

    def is_fresh(self):
        """make-style freshness for the job as a whole: every output newer than every input (in mode ``existing`` the
        var.flt.vcf files are inputs too)."""
        inputs = [self.dirs_file, self.ref_path] + [s.pileup for s in self.samples]
        names = ["consensus.fasta", "consensus_preserved.fasta"]
        if self.site_calling == "existing":
            inputs += [os.path.join(s.dir, "var.flt.vcf") for s in self.samples]
        else:
            names.append("var.flt.vcf")
        per_sample = [os.path.join(s.dir, n) for s in self.samples for n in names]
        return all(not utils.target_needs_rebuild(inputs, t) for t in list(self.outputs.values()) + per_sample)

    def open_device(self):
        torch = self.torch
        self.dev = devmod.Device(self.comm.local_rank)
        self.dev.use_torch_stream()
        # the host side's CPU budget (run.py:387-400, MaxCpuCores): the ranks of this job share the node's cores — a launcher that
        # does not export LOCAL_WORLD_SIZE still has WORLD_SIZE ranks on this one node (hot_path_batch is a single-node job)
        if self.comm.world > 1 and not os.environ.get("LOCAL_WORLD_SIZE") and not os.environ.get("SNPGPU_LOCAL_RANKS"):
            devmod.set_local_ranks(self.comm.world)
        self.cpu = devmod.cpu_budget()
        torch.cuda.set_device(self.comm.local_rank)
        # sharded over RCCL: the exchanges of the job are library calls on this context's stream (csrc/comm.hip); the gloo route of
        # the one-GPU tests, and a host whose librccl.so cannot be loaded, keep torch.distributed
        if self.comm.dist and not self.comm.one_gpu and os.environ.get("SNPGPU_COMM") != "torch":
            self.abi_comm = self.sharding.use_abi_comm(self.dev)
        # the route: ``auto`` asks the store what its budget is (creating it allocates nothing); route stream keeps no store
        if self.route_setting == "stream":
            self.pileup_route = "stream"
        else:
            self.store = self.dev.pileups(int(self.args.residentBytes or 0))
            rank_bytes = 0
            if self.route_setting == "auto" and self.site_calling in STREAM_MODES:
                for s in self.mine:
                    try:
                        rank_bytes += os.stat(s.pileup).st_size
                    except OSError:
                        pass
            self.pileup_route = resolve_pileup_route(self.route_setting, self.site_calling, rank_bytes, int(self.store.stats().budget_bytes))
            if self.pileup_route == "stream":
                self.store.close()
                self.store = None

    def close_device(self):
        if self.store is not None:
            self.store.close()
        if self.dev is not None:
            if getattr(self, "abi_comm", False):
                self.sharding.drop_abi_comm()
                self.abi_comm = False
            self.dev.close()
        self.store = self.dev = None

    @contextlib.contextmanager
    def guard(self):
        """Rank-local work between two collectives that may fail (file output): the first exception is kept and raised at the end
        of the stage, later guarded blocks are skipped, and the collectives in between still run — the peers are not left alone."""
        if self.deferred is not None:
            yield False
            return
        try:
            yield True
        except BaseException as err:                         # noqa: B902 — raised again by run_stage
            self.deferred = err

    def agree(self, err, where):
        """Collective: does any rank have a failure?  The failing rank(s) raise their own exception (its text reaches the log
        through the usual hooks); the others leave quietly with the same exit code."""
        if not self.comm.dist:
            if err is not None:
                raise err
            return
        mine = None
        if err is not None:
            code = err.code if isinstance(err, SystemExit) and isinstance(err.code, int) else (0 if isinstance(err, SystemExit) and err.code is None else 100)
            mine = (code, "%s: %s" % (type(err).__name__, err))
        every = self.comm.gather_objects(mine)
        if not any(e is not None for e in every):
            return
        self.close_device()
        self.comm.close()
        if err is not None:
            raise err
        first = next(k for k, e in enumerate(every) if e is not None)
        verbose_print("# hot_path_batch rank %d stops after %s: rank %d failed (%s)" % (self.rank, where, first, every[first][1]))
        sys.exit(every[first][0] or 100)

    def run_stage(self, stage):
        err = None
        try:
            stage(self)
            if self.deferred is not None:
                err, self.deferred = self.deferred, None
        except BaseException as e:                            # noqa: B902 — every rank must reach the agreement below
            err = e
        self.agree(err, stage.__name__)


# ==================================== stage 1: pileups -> HBM, var.flt.vcf ====================================================
def _alloc_arenas(job):
    """Host memory for the per-site results of the consensus stage, allocated AND touched while the pileups stream in.  Plain
    pageable memory: on this platform a device-to-host copy into touched pageable memory runs at the pinned rate (55 GB/s), while
    pinning a gigabyte takes 0.23 s during which every other thread's copies stand still (tools/probe/pin_probe.cpp)."""
    for k in range(2 if job.hi - job.lo > 1 else 1):
        a = np.empty(job.group_bytes, dtype=np.uint8)
        ctypes.memset(a.ctypes.data, 0, a.nbytes)      # touches the pages with the GIL released (ndarray.fill would hold it)
        job.arenas[k] = job.torch.from_numpy(a)


def _read_sample_vcf(s):
    """The records filter_regions / merge_sites read from the sample's var.flt.vcf (whoever wrote it)."""
    try:
        s.header, s.vcf_lines, s.sites = fr._read_vcf(os.path.join(s.dir, "var.flt.vcf"))
    except Exception as err:                                 # noqa: B902 — reported as this sample's error
        s.fail("Error: cannot read the VCF file of sample %s: %s: %s" % (s.name, type(err).__name__, err))


def _finish_device_sample(job, s, records, n_lines):
    """Host half of the device's call_sites for one sample (Fisher's exact test, VCF text: csrc/varscan_rows.hip), then the
    records filter_regions / merge_sites read from the file it has just written."""
    try:
        vcf_path = os.path.join(s.dir, "var.flt.vcf")
        s.n_lines = n_lines
        s.n_rows = varscan._write_vcf(vcf_path, s.pileup, records, job.vs_opts)
        s.header, s.vcf_lines, s.sites = fr._read_vcf(vcf_path)
    except Exception as err:                                 # noqa: B902 — reported as this sample's error
        s.fail("Error: call_sites failed for sample %s: %s: %s" % (s.name, type(err).__name__, err))


def _ingest_failed(s, rc, status_word):
    """The sample error for a non-zero per-file return code of the ingest, or None."""
    if rc == L.E_IO:
        return "Error: cannot open or read the pileup file %s" % s.pileup
    if rc == L.E_PILEUP:
        return "Error: call_sites failed for sample %s: ValueError: Invalid format for pileup at byte %d of %s" % (s.name, int(status_word), s.pileup)
    if rc != 0:
        return "Error: call_sites failed for sample %s (device error %d)" % (s.name, int(rc))
    return None


def _ingest_with_device_site_calling(job, todo):
    """Mode ``device``: site calling on each file while the next arrives; var.flt.vcf written by host threads as records return."""
    dev, store = job.dev, job.store
    vparams = job.vs_opts.device_params()
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(2, devmod.host_threads(16, share=4)))
    redo = []
    for b0 in range(0, len(todo), INGEST_BATCH):
        batch = todo[b0:b0 + INGEST_BATCH]
        bufs = store.ingest_buffers(len(batch), VARSCAN_CAPACITY)
        sites, counts, status, rcs, done = bufs
        first = len(store)
        failure = []

        def run_ingest(batch=batch, bufs=bufs):
            try:
                store.ingest_into([s.pileup for s in batch], vparams, VARSCAN_CAPACITY, bufs)
            except BaseException as err:                     # noqa: B902 — handed to the main thread
                failure.append(err)
                bufs[4][:] = 1

        t_call = time.perf_counter()
        th = threading.Thread(target=run_ingest)
        th.start()
        pending = list(range(len(batch)))
        futures = []
        while pending:
            still = []
            for k in pending:
                if not done[k]:
                    still.append(k)
                    continue
                s = batch[k]
                s.store_index = first + k
                if failure:
                    continue
                message = _ingest_failed(s, rcs[k], status[k, 0])
                if message:
                    s.fail(message)
                elif counts[k] > VARSCAN_CAPACITY:
                    redo.append(s)                           # more records than the shared array holds: alone, afterwards
                else:
                    futures.append(pool.submit(_finish_device_sample, job, s, sites[k, :counts[k]], int(status[k, 1])))
            pending = still
            if pending:
                time.sleep(0.0005)
        th.join()
        job.lap("1a   of which: streamed ingest calls", t_call)
        if failure:
            raise failure[0]
        t_tail = time.perf_counter()
        for fu in futures:
            fu.result()
        job.lap("1b   of which: waiting for the last var.flt.vcf files", t_tail)
    for s in redo:
        ptr, nbytes = store.get(s.store_index)
        try:
            records, n_lines = dev.varscan_dev(ptr, nbytes, vparams, capacity=4 * VARSCAN_CAPACITY) if ptr else dev.varscan_file(s.pileup, vparams)
            _finish_device_sample(job, s, records, n_lines)
        except Exception as err:                             # noqa: B902
            s.fail("Error: call_sites failed for sample %s: %s: %s" % (s.name, type(err).__name__, err))
    pool.shutdown()


def _host_site_lists(job, todo):
    """Modes ``varscan`` and ``existing``, the host's part: the VarScan jar where a var.flt.vcf is stale (``varscan``) or the check
    that the files can serve as inputs (``existing`` — nothing under samples/*/var.flt.vcf is written), then the records."""
    t_sites = time.perf_counter()
    if job.site_calling == "existing":
        for s in todo:
            message = cs.check_existing_vcf(s.pileup, os.path.join(s.dir, "var.flt.vcf"))
            if message:
                s.fail(message)
    else:
        stale = [s for s in todo if job.args.forceFlag or utils.target_needs_rebuild([s.pileup], os.path.join(s.dir, "var.flt.vcf"))]
        if stale:
            jar = cs.find_path_in_path_list("VarScan", "CLASSPATH")
            verbose_print("# %s %s  (and so on: %d samples)" % (utils.timestamp(), cs.varscan_command_line(jar or "VarScan.jar", stale[0].pileup), len(stale)))
        for s, message in zip(stale, cs.run_varscan_jar_many([(s.pileup, os.path.join(s.dir, "var.flt.vcf")) for s in stale])):
            if message:
                s.fail(message)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(2, devmod.host_threads(16, share=4))) as pool:
        list(pool.map(_read_sample_vcf, [s for s in todo if s.ok]))
    job.lap("1c   of which: var.flt.vcf files (%s) beside the ingest" % job.site_calling, t_sites)


def _pileup_unreadable(path):
    """What the ingest finds out when it opens a pileup (Opener::open_one): can it be opened for reading, is it a regular file?"""
    import stat
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return True
    try:
        return not stat.S_ISREG(os.fstat(fd).st_mode)
    finally:
        os.close(fd)


def _sites_without_ingest(job, todo):
    """Route ``stream``: no pileup byte moves in this stage.  Every pileup is opened, so that one that cannot be read fails its
    sample HERE with the ingest's message — the resident route drops such a sample before the site union, and both routes must
    write the same snplist*.txt and filtered directory lists — then the host's part of the site lists, as beside an ingest."""
    t_open = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(2, devmod.host_threads(16, share=4))) as pool:
        for s, bad in zip(todo, pool.map(_pileup_unreadable, [s.pileup for s in todo])):
            if bad:
                s.fail(_ingest_failed(s, L.E_IO, 0))
    job.lap("1a   of which: pileups opened (route stream: nothing is copied yet)", t_open)
    _host_site_lists(job, todo)


def _ingest_only(job, todo):
    """Modes ``varscan`` and ``existing``: the files are only made resident (snpgpu_pileups_ingest without parameters), in a
    helper thread; meanwhile this thread does the host's part of the site lists (_host_site_lists)."""
    store = job.store
    failure = []

    def run_ingest():
        try:
            for b0 in range(0, len(todo), INGEST_BATCH):
                batch = todo[b0:b0 + INGEST_BATCH]
                bufs = store.ingest_buffers(len(batch), 0)
                first = len(store)
                store.ingest_into([s.pileup for s in batch], None, 0, bufs)
                for k, s in enumerate(batch):
                    s.store_index = first + k
                    message = _ingest_failed(s, bufs[3][k], bufs[2][k, 0])
                    if message and s.ok:
                        s.fail(message)
        except BaseException as err:                         # noqa: B902 — handed to the main thread
            failure.append(err)

    t_call = time.perf_counter()
    th = threading.Thread(target=run_ingest)
    th.start()
    try:
        _host_site_lists(job, todo)
    finally:
        th.join()
    job.lap("1a   of which: streamed ingest calls", t_call)
    if failure:
        raise failure[0]


def _local_site_keys(job):
    """The rank's records as (contig id << 32 | position) keys over a rank-local contig table; ids are made global in the next
    stage.  Fails here — before any collective — for a position no pileup can have."""
    keys, rec_count = [], np.zeros(job.hi - job.lo, dtype=np.int64)
    job.local_names = sorted({c for s in job.mine if s.ok for c in s.sites[0]})
    for k, s in enumerate(job.mine):
        if not s.ok:
            rec_count[k] = -1                                # no var.flt.vcf: the steps below report it missing
            continue
        _, _, pos = s.sites
        if len(pos) and (pos.min() < 0 or pos.max() >= (1 << 32)):
            raise ValueError("VCF position out of range")    # as merge_sites (utils.py:1127 has no such record either)
        rec_count[k] = len(pos)
    job.rec_count_local = rec_count


def stage_ingest_and_sites(job):
    """Adds: per sample ``store_index`` and, for the samples that are still ok, ``header / vcf_lines / sites`` of its var.flt.vcf;
    ``local_names`` and ``rec_count_local`` for the gather of the next stage."""
    t0 = time.perf_counter()
    for s in job.mine:
        if utils.verify_non_empty_input_files("Pileup file", [s.pileup]) > 0:
            s.fail("Error: cannot process sample %s without its pileup file." % s.name)
    job.arena_thread = threading.Thread(target=_alloc_arenas, args=(job,))
    job.arena_thread.start()
    todo = [s for s in job.mine if s.ok]
    cs.log_site_calling_mode(job.site_calling)
    verbose_print("# pileup route: %s%s" % (job.pileup_route, " (auto)" if job.route_setting == "auto" else ""))
    if job.pileup_route == "stream":
        _sites_without_ingest(job, todo)
    elif job.site_calling == "device":
        _ingest_with_device_site_calling(job, todo)
    else:
        _ingest_only(job, todo)
    _local_site_keys(job)
    job.lap("1 ingest + site calling", t0)


# ==================================== stage 2: C1 + filter_regions + merge_sites x 2 ==========================================
def _unique_per_sample(job, keep):
    """Distinct (contig, position) pairs per sample among the records `keep` selects (the size of merge_sites' snp_set)."""
    pairs = np.unique(np.stack([job.rec_sample[keep], job.all_keys[keep]]), axis=1)
    return np.bincount(pairs[0], minlength=job.n_total)


def _site_union(job, keep, which):
    """merge_sites.py:91-117 over the records `keep`: --maxsnps sample exclusion, then the union with its carriers."""
    n_total, samples, rank = job.n_total, job.samples, job.rank
    excluded = np.zeros(n_total, bool)
    if job.ms_args.maxSnps >= 0:
        per = _unique_per_sample(job, keep)
        excluded = job.has_vcf & (per > job.ms_args.maxSnps)
        if rank == 0:
            for i in np.flatnonzero(excluded):
                verbose_print("Excluding sample %s having %d snps." % (samples[i].name, per[i]))
    inc = job.has_vcf & ~excluded
    carrier_ids = np.flatnonzero(inc)                        # carriers are indices into the INCLUDED samples, sorted-dir order
    remap = np.full(n_total, -1, dtype=np.int64)
    remap[carrier_ids] = np.arange(len(carrier_ids))
    use = keep & inc[job.rec_sample]
    if use.any():
        uniq, off, car = job.dev.merge_sites(job.all_keys[use].astype(np.uint64), remap[job.rec_sample[use]].astype(np.uint32))
    else:
        uniq, off, car = np.zeros(0, np.uint64), np.zeros(1, np.uint32), np.zeros(0, np.uint32)
    if rank == 0:
        verbose_print("Found %d snp positions across %d sample vcf files." % (len(uniq), n_total))
        ms.write_snplist(job.outputs[which], job.contigs, uniq, off, car, [samples[i].name for i in carrier_ids])
        with open(job.filtered1 if which == "snplist" else job.filtered2, "w") as f:
            for d in job.unsorted_dirs:                      # original order (merge_sites.py:127-131)
                if not excluded[job.dir_index[d]]:
                    f.write("%s\n" % d)
    return uniq.astype(np.int64), excluded


def stage_site_union_and_regions(job):
    """Collectives first (contig names, record keys, record counts), then identical work on every rank.  Adds: ``contigs``,
    ``all_keys`` / ``rec_off`` / ``rec_sample`` (every sample's records), ``has_vcf``, ``list1`` / ``list2`` (the two site unions),
    ``excluded1`` / ``excluded2``, per sample ``removed``, and the futures of the split VCF writers (``split_files``)."""
    torch, comm, sharding = job.torch, job.comm, job.sharding
    n_total, samples, mine, dev = job.n_total, job.samples, job.mine, job.dev
    t0 = time.perf_counter()
    # every rank learns every sample's records: contig names as objects (a few strings), the records as one all-gather
    job.contigs = contigs = sorted({c for names in comm.gather_objects(job.local_names) for c in names})
    cid = {c: i for i, c in enumerate(contigs)}
    keys_local = []
    for s in mine:
        if s.ok:
            names, cidx, pos = s.sites
            lut = np.asarray([cid[c] for c in names] + [0], dtype=np.int64)
            keys_local.append((lut[cidx.astype(np.int64)] << 32) | pos)
    keys_local = np.concatenate(keys_local) if keys_local else np.zeros(0, np.int64)
    if comm.dist:
        dv = "cpu" if comm.one_gpu else "cuda"
        all_keys, _ = sharding.all_gather_varlen(torch.from_numpy(keys_local).to(dv))
        all_cnt, _ = sharding.all_gather_varlen(torch.from_numpy(job.rec_count_local).to(dv))
        all_keys, all_cnt = all_keys.cpu().numpy(), all_cnt.cpu().numpy()
    else:
        all_keys, all_cnt = keys_local, job.rec_count_local
    job.all_keys = all_keys
    job.has_vcf = has_vcf = all_cnt >= 0
    cnt0 = np.maximum(all_cnt, 0)
    job.rec_off = rec_off = np.zeros(n_total + 1, dtype=np.int64)
    np.cumsum(cnt0, out=rec_off[1:])
    job.rec_sample = rec_sample = np.repeat(np.arange(n_total, dtype=np.int64), cnt0)
    rec_cid = (all_keys >> 32).astype(np.uint32)
    rec_pos = all_keys & 0xFFFFFFFF
    n_bad = int((~has_vcf).sum())
    if n_bad == n_total:                                     # every rank sees the same counts: all leave, rank 0 says why
        if job.rank == 0:
            utils.global_error("Error: all %d VCF files were missing or empty." % n_bad)
        sys.exit(100)
    elif n_bad > 0:
        # a sample without var.flt.vcf.  Under StopOnSampleError the pipeline ends here, as it does when the call_sites array or
        # merge_sites reports it (run.py stops at the first failed step) — on EVERY rank: each says what failed for its own samples
        if utils._stop_on_sample_error():
            for s in mine:
                if not s.ok:
                    utils.sample_error(s.error, continue_possible=True)          # (exits 100)
            if job.rank == 0:
                utils.sample_error("Error: %d VCF files were missing or empty." % n_bad, continue_possible=True)
            sys.exit(100)
        if job.rank == 0:
            utils.sample_error("Error: %d VCF files were missing or empty." % n_bad, continue_possible=True)

    every = np.ones(len(all_keys), dtype=bool)
    job.lap("2a   of which: gathering the records", t0)
    t2 = time.perf_counter()
    job.list1, job.excluded1 = _site_union(job, every, "snplist")
    job.lap("2b   of which: site union + snplist.txt", t2)
    t2 = time.perf_counter()

    # filter_regions (filter_regions.py:205-383): dense windows + contig edges -> merged bad regions -> classification of
    # every record; mode all unions the regions over the samples, mode each keeps them per sample; outgroup samples bypass
    fr_args = job.fr_args
    outgroup = set()
    if fr_args.outGroupFile is not None:
        if utils.verify_non_empty_input_files("File of outgroup samples", [fr_args.outGroupFile]) > 0:
            utils.global_error(None)
        with open(fr_args.outGroupFile, "r") as f:
            outgroup = {line.rstrip() for line in f}
    try:
        contig_lengths = utils.read_fasta_lengths(job.ref_path)
    except (IOError, OSError, UnicodeDecodeError):
        utils.global_error("Error: cannot open the reference fastq file, or fail to read the contigs in the reference fastq file.")
    job.is_out = is_out = np.asarray([s.name in outgroup for s in samples], dtype=bool)
    filt = has_vcf & ~is_out                                 # the samples that take part in the region step
    filt_ids = np.flatnonzero(filt)
    part_rank = np.full(n_total, -1, dtype=np.int64)
    part_rank[filt_ids] = np.arange(len(filt_ids))
    takes_part = filt[rec_sample]
    job.lap("2c   of which: (records laid out)", t2)
    t2 = time.perf_counter()
    removed = np.zeros(len(all_keys), dtype=bool)
    removed[takes_part] = fr.removed_flags(dev, contigs, contig_lengths, part_rank[rec_sample[takes_part]], rec_cid[takes_part], rec_pos[takes_part],
                                           len(filt_ids), fr_args.edgeLength, fr_args.maxSnpsList, fr_args.windowSizeList, per_sample=fr_args.mode == "each")
    preserved = every & ~removed
    job.lap("2d   of which: dense windows, region merge, classification", t2)
    t2 = time.perf_counter()
    job.list2, job.excluded2 = _site_union(job, preserved, "snplist_p")
    job.lap("2e   of which: preserved site union + snplist_preserved.txt", t2)
    t2 = time.perf_counter()
    # the split VCF files of this rank's samples: written by host threads while the consensus stage keeps the device busy
    job.split_pool = concurrent.futures.ThreadPoolExecutor(max_workers=devmod.host_threads(4))
    job.split_files = []
    for s in mine:
        if not s.ok:
            continue
        vcf_path = os.path.join(s.dir, "var.flt.vcf")
        if is_out[s.index]:
            job.split_files.append(job.split_pool.submit(fr.write_outgroup_preserved_and_removed_vcf_files, vcf_path, s.header))
        else:
            s.removed = removed[rec_off[s.index]:rec_off[s.index + 1]]
            job.split_files.append(job.split_pool.submit(fr.write_preserved_and_removed_vcf_files, vcf_path, s.header, s.vcf_lines, s.removed))
    job.lap("2f   of which: var.flt_preserved / _removed.vcf files handed to writer threads", t2)
    job.lap("2 site union + region filter", t0)


# ==================================== stage 3: both consensus flows from one scan + call ======================================
class _Flows(object):
    """What the consensus stage works with: the site set (snplist.txt, the rank's own removed positions, what only
    snplist_preserved.txt has), the column maps of the two flows, device and host result arrays."""


def _prepare_flows(job):
    torch, dev, mine = job.torch, job.dev, job.mine
    cc_args = job.cc_args
    fl = _Flows()
    list1, list2, all_keys, rec_off = job.list1, job.list2, job.all_keys, job.rec_off
    # the site set: snplist.txt, plus removed positions of this rank's samples that are not in it (a sample merge_sites
    # excluded for --maxsnps is still called, run.py:704-718, and its exclude list is parsed: call_consensus.py:147-151),
    # plus what snplist_preserved.txt has and snplist.txt has not: with --maxsnps a sample can be out of the first list for its
    # var.flt.vcf and in the second for its shorter var.flt_preserved.vcf (found by tools/fuzz_jobs.py)
    fl.own_removed = {s.index: (all_keys[rec_off[s.index]:rec_off[s.index + 1]][s.removed] if (s.ok and s.removed is not None) else np.zeros(0, np.int64))
                      for s in mine}
    extra = np.setdiff1d(np.concatenate(list(fl.own_removed.values())) if fl.own_removed else np.zeros(0, np.int64), list1)
    set_keys = list1
    for more in (extra, np.setdiff1d(list2, list1)):
        if len(more):
            set_keys = np.union1d(set_keys, more)
    fl.set_keys = set_keys
    fl.S = S = len(set_keys)
    fl.S1, fl.S2 = S1, S2 = len(list1), len(list2)
    cols1 = np.searchsorted(set_keys, list1).astype(np.uint32)
    cols2 = np.searchsorted(set_keys, list2).astype(np.uint32)
    fl.in1 = in1 = np.zeros(S, dtype=np.uint8)
    in1[cols1] = 1
    fl.in2 = in2 = np.zeros(S, dtype=np.uint8)
    in2[cols2] = 1
    col_of2 = np.full(S, -1, dtype=np.int32)
    col_of2[cols2] = np.arange(len(cols2), dtype=np.int32)
    fl.contig_bytes = [c.encode("utf-8") for c in job.contigs]
    # Contig names that are not plain ASCII (just names to the reference, which reads its files as text): the scan's byte tests are
    # ASCII-only, so the device sees every name escaped (utf8_names: injective, order-preserving, plain names unchanged) — in the
    # site set here, and in a copy of the pileups that spell such names (made when the scan meets one, _consensus_group) — while
    # everything that is written keeps the names as they are.
    from . import utf8_names
    fl.device_contigs = [utf8_names.escape_name(c) for c in fl.contig_bytes]
    fl.escaped = fl.device_contigs != fl.contig_bytes
    fl.ss = devmod.SiteSet.from_arrays(dev, fl.contig_bytes, set_keys.astype(np.uint64), in1 * np.uint8(L.SITE_IN_SNPLIST),
                                       device_contigs=fl.device_contigs if fl.escaped else None)
    fl.identity1 = len(set_keys) == len(list1)
    fl.prm = devmod.make_params(cc_args.minBaseQual, cc_args.minConsFreq, cc_args.minConsDpth, cc_args.minConsStrdDpth, cc_args.minConsStrdBias)
    # collect_metrics by-products (call_consensus --amdMetricsRefFasta, given through CallConsensus_ExtraParams): the depth
    # column is summed by the same scan, the gaps are counted in the rows that are written anyway
    fl.metrics_ref = getattr(cc_args, "amdMetricsRefFasta", None)
    fl.metrics_ref_len = sum(utils.read_fasta_lengths(fl.metrics_ref).values()) if fl.metrics_ref else 0
    fl.want_depth = bool(fl.metrics_ref) or job.collect_metrics     # the depth column is summed by the scan for either of them
    fl.filters_desc = vcf_writer.filter_descriptions(cc_args.minConsFreq, cc_args.minConsDpth, cc_args.minConsStrdDpth, cc_args.minConsStrdBias)
    fl.filter_names = [n for n, _ in fl.filters_desc]
    fl.d_cols1, fl.d_cols2 = torch.from_numpy(cols1.astype(np.int32)).cuda(), torch.from_numpy(cols2.astype(np.int32)).cuda()
    fl.d_col_of2 = torch.from_numpy(col_of2).cuda()
    fl.d_col_of1 = torch.from_numpy(np.where(in1 != 0, np.cumsum(in1, dtype=np.int64) - 1, -1).astype(np.int32)).cuda()
    fl.d_in12_u8 = torch.from_numpy((in1 | in2).astype(np.uint8)).cuda()     # 1: a position every sample of the job is asked about
    fl.d_err = torch.zeros(4, dtype=torch.int32, device="cuda")
    job.callable_ = callable_ = [s for s in mine if s.ok]
    fl.n_local = n_local = len(callable_)
    job.rows1 = torch.full((max(n_local, 1), max(S1, 1)), 0x2D, dtype=torch.uint8, device="cuda")     # the consensus rows, for stage 4
    job.rows2 = torch.full((max(n_local, 1), max(S2, 1)), 0x2D, dtype=torch.uint8, device="cuda")
    job.row_ok = np.zeros(n_local, dtype=bool)
    want_vcf = job.want_vcf
    fl.per_sample_bytes = max(S1, 1) + max(S2, 1) + 2 * max(S, 1) + 8 * max(S, 1) + 32 + (128 * max(S, 1) if want_vcf else 0) + 64
    fl.group = max(1, min(256, job.group_bytes // fl.per_sample_bytes))
    if n_local >= 32:
        # at least two groups — four from 64 samples on: the files of one are written while the next is on the device, and what is
        # left to wait for at the end is the last group's files (1.25 GB of VCF text for 125 samples: a quarter of it instead of half)
        fl.group = min(fl.group, (n_local + 3) // 4 if n_local >= 64 else (n_local + 1) // 2)
    fl.g_alloc = g_alloc = min(fl.group, max(n_local, 1))
    fl.d_base = torch.empty((g_alloc, max(S, 1)), dtype=torch.uint8, device="cuda")
    fl.d_filt = torch.empty((g_alloc, max(S, 1)), dtype=torch.uint8, device="cuda")
    fl.d_filt2 = torch.empty((g_alloc, max(S, 1)), dtype=torch.uint8, device="cuda")
    fl.d_line = torch.zeros((g_alloc, max(S, 1)), dtype=torch.int64, device="cuda")
    fl.d_status = torch.empty((g_alloc, 4), dtype=torch.int64, device="cuda")
    fl.d_counts = torch.empty((g_alloc, max(S, 1), 128), dtype=torch.uint8, device="cuda") if want_vcf else None
    fl.host_sets = [None, None]
    fl.vcf_date = datetime.datetime.now()
    return fl


def _host_set(job, fl, k):
    """Result arrays of one group, carved out of arena k (allocated while the pileups were streaming in)."""
    torch = job.torch
    S, S1, S2, g_alloc = fl.S, fl.S1, fl.S2, fl.g_alloc
    need = g_alloc * fl.per_sample_bytes + 4096
    if job.arenas[k] is None or job.arenas[k].numel() < need:
        job.arenas[k] = torch.from_numpy(np.zeros(need, dtype=np.uint8))
    at = [0]

    def carve(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        start = (at[0] + 63) // 64 * 64
        at[0] = start + nbytes
        return job.arenas[k][start:start + nbytes].view(dtype).view(*shape)

    return {"g": g_alloc,
            "status": carve((g_alloc, 4), torch.int64),
            "line": carve((g_alloc, max(S, 1)), torch.int64),
            "counts": carve((g_alloc, max(S, 1), 128), torch.uint8) if job.want_vcf else None,
            "base1": carve((g_alloc, max(S1, 1)), torch.uint8),
            "base2": carve((g_alloc, max(S2, 1)), torch.uint8),
            "filt1": carve((g_alloc, max(S, 1)), torch.uint8),
            "filt2": carve((g_alloc, max(S, 1)), torch.uint8)}


def _write_group(job, fl, part, hs, vcf_later, spill=None):
    """FASTA + VCF files of one group, both flows (host threads inside the library); returns the samples that failed."""
    cc_args, want_vcf = job.cc_args, job.want_vcf
    S, S1, S2 = fl.S, fl.S1, fl.S2
    jobs, owners = [], []
    counts_np = hs["counts"].numpy().view(devmod.COUNTS_DTYPE).reshape(hs["g"], max(S, 1)) if want_vcf else None
    for k, s in enumerate(part):
        if not s.ok:
            continue
        for flow in (1, 2):
            seq = (hs["base1"] if flow == 1 else hs["base2"]).numpy()[k, :(S1 if flow == 1 else S2)]
            item = {"fasta_path": os.path.join(s.dir, "consensus.fasta" if flow == 1 else "consensus_preserved.fasta"),
                    "fasta_id": s.name.encode("utf-8"), "sequence": seq}
            if want_vcf and s.index not in vcf_later:
                hdr = "\n".join(vcf_writer.header_lines(s.name, fl.filters_desc, cc_args.vcfRefName, now=fl.vcf_date)) + "\n"
                item.update({"vcf_path": os.path.join(s.dir, "consensus.vcf" if flow == 1 else "consensus_preserved.vcf"),
                             "vcf_header": hdr.encode("utf-8"), "counts": counts_np[k], "line_off": hs["line"].numpy()[k].view(np.uint64),
                             "row_filters": (hs["filt1"] if flow == 1 else hs["filt2"]).numpy()[k],
                             "site_in_flow": fl.in1 if flow == 1 else fl.in2})
            jobs.append(item)
            owners.append(s)
    res = devmod.write_consensus_files(jobs, fl.ss, fl.filter_names, cc_args.vcfPreserveRefCase, cc_args.vcfFailedSnpGt, n_threads=job.args.writerThreads,
                                       spill=spill)
    if job.collect_metrics:                                  # kept for stage_collect_metrics: no pileup and no FASTA is read again
        st_h = hs["status"].numpy()
        for k, s in enumerate(part):
            if s.ok:
                job.metrics_known[s.dir] = {"depth_sum": int(st_h[k, 3]) & 0xFFFFFFFFFFFFFFFF,
                                            "missingPos": int(np.count_nonzero(hs["base1"].numpy()[k, :S1] == 0x2D)),
                                            "missingPosPreserved": int(np.count_nonzero(hs["base2"].numpy()[k, :S2] == 0x2D))}
    if fl.metrics_ref:                                       # as call_consensus._record_metrics does for the two flows, in their order
        st_h = hs["status"].numpy()
        for k, s in enumerate(part):
            if not s.ok:
                continue
            name = os.path.basename(cc_args.amdMetricsFile) if cc_args.amdMetricsFile else "metrics"
            depth_sum = int(st_h[k, 3]) & 0xFFFFFFFFFFFFFFFF
            ave = {"avePileupDepth": "%.2f" % (float(depth_sum) / float(fl.metrics_ref_len))} if depth_sum > 0 and fl.metrics_ref_len > 0 else {}
            for key, row, n in (("missingPos", hs["base1"], S1), ("missingPosPreserved", hs["base2"], S2)):
                updates = {key: str(int(np.count_nonzero(row.numpy()[k, :n] == 0x2D)))}
                updates.update(ave)
                utils.update_properties(os.path.join(s.dir, name), updates, keep_mtime=True)
    bad = []
    for s, item, (rc, _) in zip(owners, jobs, res):
        if rc == L.E_UNSUPPORTED:
            bad.append((s, "Error: call_consensus failed for sample %s: ValueError: a position has more than %d distinct symbols" % (s.name, L.MAX_SYMS)))
        elif rc != 0:
            bad.append((s, "Error: cannot write %s" % item["fasta_path"]))
    return bad


def _wanted_mask(fl, s):
    """The slots of the site set THIS sample's two call_consensus runs are asked about (call_consensus.py:147-151): snplist.txt,
    snplist_preserved.txt and its own removed positions.  The set also holds other samples' removed positions; the reference
    builds no Record at those for this sample."""
    wanted = (fl.in1 | fl.in2).astype(bool)
    own = fl.own_removed[s.index]
    if len(own):
        wanted[np.searchsorted(fl.set_keys, own)] = True
    return wanted


def _check_repeated_lines(job, fl, s, status_row):
    """The pileup repeats a listed position.  The last line of a position is the one that counts for the consensus
    (call_consensus.py:171-176) and that is what the device returned; but the reference builds a Record from every such line —
    it ends at the first it cannot build — and writes a consensus.vcf row for each.  The all-lines pass looks at them now,
    with the sample's OWN positions flagged as listed.  Returns the exception the reference would end with, or None."""
    wanted = _wanted_mask(fl, s)
    own_set = devmod.SiteSet.from_arrays(job.dev, fl.contig_bytes, fl.set_keys.astype(np.uint64), wanted.astype(np.uint8) * np.uint8(L.SITE_IN_SNPLIST),
                                         device_contigs=fl.device_contigs if fl.escaped else None)
    copy = None
    try:
        if getattr(s, "names_escaped", False):                 # (the file the device can read: its names escaped)
            from . import utf8_names
            copy = utf8_names.escaped_copy(s.pileup)
        _, line_flags, line_counts = job.dev.call_all_lines(own_set, copy or s.pileup, fl.prm, check=False)
        err, _ = devmod.Device.site_error(devmod.ConsensusResult(None, None, line_counts[line_flags != 0], status_row))
    except (devmod.PileupFormatError, devmod.PileupIOError) as e:
        err = e
    finally:
        own_set.close()
        if copy:
            os.unlink(copy)
    return err


def _consensus_group(job, fl, g0, part, hs, vcf_again, vcf_later):
    """Device work of one group of samples and its results on the way to the host.  Returns (chk, rest, t_mark): per sample
    [malformed line at one of ITS positions, listed positions with a line, positions with a spill record]."""
    torch, dev, store, args = job.torch, job.dev, job.store, job.args
    S, S1, S2, want_vcf = fl.S, fl.S1, fl.S2, job.want_vcf
    ss, prm = fl.ss, fl.prm
    d_base, d_filt, d_filt2, d_line, d_status, d_counts = fl.d_base, fl.d_filt, fl.d_filt2, fl.d_line, fl.d_status, fl.d_counts
    t_g = time.perf_counter()
    g = len(part)
    one_launch = False                                        # the whole group in ONE call launch: then the launch's pass counts are the group's
    streamed = job.pileup_route == "stream"
    if streamed:
        # nothing is resident: the group is ONE streamed call whose kernels write the group's rows where the flow kernels read them
        # (snpgpu_call_consensus_files_dev) — the only time these pileups cross the link.  With an empty site set nothing is
        # scanned, as on the resident route.
        if S:
            status, rcs, st = dev.call_consensus_files_dev(ss, [s.pileup for s in part], prm, d_base.data_ptr(), d_filt.data_ptr(),
                                                           d_counts=d_counts.data_ptr() if want_vcf else 0, d_line_off=d_line.data_ptr(),
                                                           want_depth_sum=fl.want_depth)
            d_status[:g] = torch.from_numpy(status.view(np.int64)).cuda()
            job.h2d_extra += int(st.bytes)
            job.stream_stats["file_bytes"] += int(st.bytes)
            job.stream_stats["files"] += g
            job.stream_stats["seconds"] += float(st.seconds)
            job.stream_stats["readers"] = max(job.stream_stats["readers"], int(st.n_readers))
            for s, rc in zip(part, rcs):
                if int(rc) == L.E_IO:                         # (readable in stage 1, not any more)
                    s.fail(_ingest_failed(s, L.E_IO, 0))
        else:
            d_status[:g] = torch.tensor([-1, 0, 0, 0], dtype=torch.int64, device="cuda")
    resident = [] if streamed else [(k, s) + store.get(s.store_index) for k, s in enumerate(part)]
    res_idx = [k for k, s, ptr, _ in resident if ptr]
    if res_idx and S:
        # resident samples first in the group's arrays would need a permutation: call them in place, sample by sample
        # position, with one launch over all resident ones
        ptrs = [ptr for _, _, ptr, _ in resident if ptr]
        sizes = [n for _, _, ptr, n in resident if ptr]
        if len(res_idx) == g:
            one_launch = g <= 256 and 8 * S * g <= (1 << 30)  # (what snpgpu_call_consensus_many_dev puts into one launch)
            dev.call_consensus_many_dev(ss, ptrs, sizes, prm, d_base.data_ptr(), d_filt.data_ptr(), d_status.data_ptr(),
                                        d_counts=d_counts.data_ptr() if want_vcf else 0, d_line_off=d_line.data_ptr(),
                                        want_depth_sum=fl.want_depth)
        else:
            _call_scattered(dev, ss, prm, res_idx, ptrs, sizes, d_base, d_filt, d_status, d_counts, d_line, S, want_vcf, torch,
                            want_depth_sum=fl.want_depth)
    elif res_idx:
        d_status[:g] = torch.tensor([-1, 0, 0, 0], dtype=torch.int64, device="cuda")
    rest = [(k, s) for k, s, ptr, _ in resident if not ptr]

    def put_rows(k, r):                                       # the result of a streamed sample into row k of the group's arrays
        d_status[k] = torch.from_numpy(r.status.astype(np.int64)).cuda()
        if S:
            d_base[k, :S] = torch.from_numpy(r.bases).cuda()
            d_filt[k, :S] = torch.from_numpy(r.filters).cuda()
            d_line[k, :S] = torch.from_numpy(r.line_offsets.astype(np.int64)).cuda()
            if want_vcf:
                d_counts[k, :S] = torch.from_numpy(r.counts.view(np.uint8).reshape(S, 128)).cuda()
    if rest:
        # files that did not fit the memory budget: streamed again (the only pileups that cross the link twice)
        results, rcs, st = dev.call_consensus_files(ss, [s.pileup for _, s in rest], prm, want_counts=want_vcf, want_line_offsets=True,
                                                    want_depth_sum=fl.want_depth)
        job.h2d_extra += int(st.bytes)
        for (k, s), rc, r in zip(rest, rcs, results):
            if int(rc) == L.E_IO:
                s.fail("Error: cannot open or read the pileup file %s" % s.pileup)
            put_rows(k, r)
    if fl.escaped and S:
        # Some contig name of the job is not plain ASCII.  A pileup that spells such a name stops the scan at its first byte >= 0x80
        # (scan code 3); the device gets a copy of that file with every name escaped, as the site set has them, and the sample's
        # rows come from there (call_consensus does the same for one sample).  Characters >= 0x80 outside the name column stay
        # refused (utf8_names.Refused: the sample keeps its scan error), a file that is not valid UTF-8 too.
        from . import utf8_names
        st_now = d_status[:g].cpu().numpy()
        again = [(k, s) for k, s in enumerate(part) if s.ok and (int(st_now[k, 0]) & 0xFF) == 3 and (int(st_now[k, 0]) & 0xFFFFFFFFFFFFFFFF) != 0xFFFFFFFFFFFFFFFF]
        copies = []
        try:
            for k, s in again:
                try:
                    copies.append((k, s, utf8_names.escaped_copy(s.pileup)))
                except (utf8_names.Refused, UnicodeDecodeError, OSError):
                    pass                                      # (its scan error stands)
            if copies:
                one_launch = False
                results, rcs, st = dev.call_consensus_files(ss, [c for _, _, c in copies], prm, want_counts=want_vcf, want_line_offsets=True,
                                                            want_depth_sum=fl.want_depth)
                job.h2d_extra += int(st.bytes)
                for (k, s, _), rc, r in zip(copies, rcs, results):
                    if int(rc) == L.E_IO:
                        continue
                    s.names_escaped = True
                    put_rows(k, r)
        finally:
            for _, _, c in copies:
                try:
                    os.unlink(c)
                except OSError:
                    pass
    # the preserved flow (and, when the set is wider than snplist.txt, the columns of the full flow) on the device
    excl = [np.searchsorted(fl.set_keys, fl.own_removed[s.index]).astype(np.uint32) for s in part]
    eoff = np.zeros(g + 1, dtype=np.int32)
    np.cumsum([len(e) for e in excl], out=eoff[1:])
    d_eoff = torch.from_numpy(eoff).cuda()
    d_eslots = torch.from_numpy(np.concatenate(excl).astype(np.int32) if eoff[-1] else np.zeros(1, np.int32)).cuda()
    d_b2 = job.rows2[g0:g0 + g]
    dev.region_flow_dev(d_base.data_ptr(), d_filt.data_ptr(), d_line.data_ptr(), g, S, fl.d_cols2.data_ptr(), fl.d_col_of2.data_ptr(), S2,
                        d_eoff.data_ptr(), d_eslots.data_ptr() if eoff[-1] else 0, d_b2.data_ptr() if S2 else 0, d_filt2.data_ptr(), fl.d_err.data_ptr())
    if fl.identity1:
        if S1:
            job.rows1[g0:g0 + g, :S1] = d_base[:g, :S1]
    else:
        d_nofilt = torch.empty_like(d_filt2)
        d_e0 = torch.zeros(g + 1, dtype=torch.int32, device="cuda")
        dev.region_flow_dev(d_base.data_ptr(), d_filt.data_ptr(), d_line.data_ptr(), g, S, fl.d_cols1.data_ptr(), fl.d_col_of1.data_ptr(), S1,
                            d_e0.data_ptr(), 0, job.rows1[g0:g0 + g].data_ptr() if S1 else 0, d_nofilt.data_ptr(), fl.d_err.data_ptr())
    # results to the host
    if args.verbose >= 2:
        torch.cuda.current_stream().synchronize()
        job.lap("3a   of which: scan + call + flows on the device", t_g)
        t_g = time.perf_counter()
    # per sample, for the checks below — over the positions THAT SAMPLE is asked about (snplist.txt, snplist_preserved.txt, its own
    # removed positions; the set also holds other samples' removed positions, where the reference builds no Record for this one):
    # a malformed line at one of them?  how many of the set's positions have a line?  how many have a spill record?
    d_chk = None
    if S:
        # (k_group_check, csrc/comm.hip: one workgroup per sample; rounds 2-4 did this with half a dozen ATen kernels per group)
        d_chk = torch.empty((g, 3), dtype=torch.int64, device="cuda")
        own = bool(eoff[-1]) and not fl.identity1             # (with the set == snplist.txt every own position is in it already)
        dev.group_check_dev(0 if want_vcf else d_filt.data_ptr(), d_counts.data_ptr() if want_vcf else 0, d_line.data_ptr(), fl.d_in12_u8.data_ptr(),
                            d_eoff.data_ptr() if own else 0, d_eslots.data_ptr() if own else 0, g, S, d_chk.data_ptr())
    hs["status"][:g].copy_(d_status[:g], non_blocking=True)
    if S1:
        hs["base1"][:g, :S1].copy_(job.rows1[g0:g0 + g, :S1], non_blocking=True)
    if S2:
        hs["base2"][:g, :S2].copy_(job.rows2[g0:g0 + g, :S2], non_blocking=True)
    if S:
        hs["filt1"][:g, :S].copy_(d_filt[:g, :S], non_blocking=True)
        hs["filt2"][:g, :S].copy_(d_filt2[:g, :S], non_blocking=True)
        hs["line"][:g, :S].copy_(d_line[:g, :S], non_blocking=True)
        if want_vcf:
            hs["counts"][:g, :S].copy_(d_counts[:g, :S], non_blocking=True)
    chk = d_chk.cpu().numpy() if S else np.zeros((g, 3), dtype=np.int64)      # (the stream is idle after this)
    group_spill = None
    if S and chk[:, 2].any():
        # positions with more than 8 distinct symbols: their spill records belong to ONE library call — there is one
        # when the whole group was resident or the whole group was one streamed call (route stream); a sample of a mixed
        # group goes back to the per-sample command
        if not rest:
            group_spill = dev.read_symbol_spill()
        else:
            for k, s in enumerate(part):
                if s.ok and chk[k, 2]:                       # its consensus is as good as any; its VCF rows need the spill of a call of its own
                    vcf_again.append(s)
                    vcf_later.add(s.index)
    torch.cuda.current_stream().synchronize()
    if S and one_launch and not rest:
        # which call kernel took how many of the group's lines (the device is idle here: the read-back costs one small copy).  The
        # library keeps the figures of its last launch only, so a group that took several launches (samples streamed again, escaped
        # copies, scattered calls) is counted under "groups_not_counted" instead.  Lines under "wave" are off the fast path: over
        # 512 bytes, or malformed.
        passes = dev.call_pass_counts()
        for k, v in passes.items():
            job.call_passes[k] = job.call_passes.get(k, 0) + v
        if args.verbose >= 2:
            verbose_print("#   call passes, samples %d-%d: %s" % (g0, g0 + g - 1, "  ".join("%s %d" % (k, passes[k]) for k in devmod.Device.CALL_PASS_NAMES)))
    elif S:
        job.call_passes["groups_not_counted"] = job.call_passes.get("groups_not_counted", 0) + 1
    job.lap("3b   of which: results to the host" if args.verbose >= 2 else "3ab  of which: device work + results to the host", t_g)
    return chk, group_spill


def _check_group(job, fl, g0, part, hs, chk, vcf_again):
    """What the per-sample CLI raises for: malformed chrom / position columns anywhere, a malformed line at a listed position, a
    line of a repeated position that no Record can be built from.  Marks the rows that stand (``row_ok``)."""
    S = fl.S
    st_np = hs["status"].numpy()[:len(part)]
    for k, s in enumerate(part):
        if not s.ok:
            continue
        w0 = int(st_np[k, 0]) & 0xFFFFFFFFFFFFFFFF
        if w0 != 0xFFFFFFFFFFFFFFFF:
            s.fail("Error: call_consensus failed for sample %s: malformed pileup %s at byte offset %d" % (s.name, s.pileup, (w0 >> 8) - 1))
            continue
        if S and chk[k, 0]:
            s.fail("Error: call_consensus failed for sample %s: malformed pileup line at a listed position" % s.name)
            continue
        if S and int(st_np[k, 2]) > int(chk[k, 1]):
            # more matching lines than positions with a line: a position comes twice (a sorted pileup never gets here).  The VCF
            # files of such a sample are written by the per-sample command once the job's own files are done
            err = _check_repeated_lines(job, fl, s, st_np[k])
            if err is not None:
                s.fail("Error: call_consensus failed for sample %s: %s" % (s.name, err))
                continue
            if job.want_vcf and s not in vcf_again:
                vcf_again.append(s)
        job.row_ok[g0 + k] = True


def stage_consensus(job):
    """No collective in this stage.  Adds: ``flows`` (site set, column maps), ``callable_`` (the rank's samples that got this far),
    ``rows1`` / ``rows2`` (device: consensus rows of both flows), ``row_ok``, ``vcf_again``."""
    t0 = time.perf_counter()
    job.flows = fl = _prepare_flows(job)
    job.lap("3-   of which: site set", t0)
    callable_, n_local, group = job.callable_, fl.n_local, fl.group
    job.arena_thread.join()
    writer = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    pending_write = None
    job.vcf_again = vcf_again = []                           # samples whose VCF files the per-sample command writes at the end
    vcf_later = set()                                        # ... of them, those whose group must not write a VCF meanwhile
    write_failures = []
    for g0 in range(0, n_local, group):
        part = callable_[g0:g0 + group]
        which = (g0 // group) & 1
        if fl.host_sets[which] is None:
            fl.host_sets[which] = _host_set(job, fl, which)
        hs = fl.host_sets[which]
        for attempt in range(5):
            try:
                chk, group_spill = _consensus_group(job, fl, g0, part, hs, vcf_again, vcf_later)
                break
            except devmod.SpillOverflow:                     # more positions with a spill record than the arena held: it has grown, again
                if attempt == 4:
                    raise
        t_g = time.perf_counter()
        _check_group(job, fl, g0, part, hs, chk, vcf_again)
        job.lap("3c   of which: status checks", t_g)
        t_g = time.perf_counter()
        if pending_write is not None:
            write_failures.extend(pending_write.result())
        pending_write = writer.submit(_write_group, job, fl, part, hs, vcf_later, group_spill)
        job.lap("3d   of which: waiting for the previous group's files", t_g)
    t_g = time.perf_counter()
    if pending_write is not None:
        write_failures.extend(pending_write.result())
    writer.shutdown()
    job.lap("3e   of which: waiting for the last group's files", t_g)
    for s, msg in write_failures:
        s.fail(msg)
        job.row_ok[callable_.index(s)] = False
    if int(fl.d_err[0]) != 0:
        raise RuntimeError("an exclude slot fell outside the site set")
    t_g = time.perf_counter()
    for fu in job.split_files:
        fu.result()
    job.split_pool.shutdown()
    job.lap("3f   of which: waiting for the split VCF files of step 2", t_g)
    job.lap("3 consensus, both flows", t0)


# ==================================== stage 4: matrices, distances, top-level files ===========================================
def _close_rows(torch, dev, d_matrix, n, row_stride, row_lo, row_hi, threshold):
    """Rows [row_lo, row_hi) of a device distance matrix (row i at d_matrix + 4 * i * row_stride) thresholded there: (entries per
    row, columns, distances) as host arrays.  The first call has room for 32 entries per row (an outbreak threshold keeps a few):
    only a denser answer costs a second call with the room the first one asked for."""
    rows = row_hi - row_lo
    row_off = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    capacity = max(32 * rows, 1 << 16)
    while True:
        col = torch.zeros(capacity, dtype=torch.int32, device="cuda")
        dist = torch.zeros(capacity, dtype=torch.int32, device="cuda")
        total = dev.close_pairs_dev(d_matrix, n, row_stride, row_lo, row_hi, threshold, capacity, row_off.data_ptr(), col.data_ptr(), dist.data_ptr())
        if total <= capacity:
            break
        capacity = total
    return np.diff(row_off.cpu().numpy()).astype(np.uint64), col[:total].cpu().numpy().view(np.uint32), dist[:total].cpu().numpy()


def close_rows_over_ranks(torch, dev, comm, bands, dmat, band, n, threshold):
    """The entries <= threshold of the whole n x n distance matrix as a CSR (row_off, col, dist) on rank 0, None on the others.
    With one rank: from `dmat` (pitch bands.n_padded).  With several: `band` holds the complete rows of this rank's band after
    bands.exchange (the same pitch); each rank thresholds those on the device — the kernel is given where row 0 WOULD lie in front of
    the band, and the band's own row range — and the pieces are gathered in rank order, which is row order."""
    if band is not None:
        blo, bhi = bands.band_rows(comm.rank)
        parts = comm.gather_objects(_close_rows(torch, dev, band.data_ptr() - blo * bands.n_padded * 4, n, bands.n_padded, blo, bhi, threshold))
    else:
        parts = [_close_rows(torch, dev, dmat.data_ptr(), n, max(bands.n_padded, 1), 0, n, threshold)]
    if comm.rank != 0:
        return None
    row_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.concatenate([p[0] for p in parts]), out=row_off[1:])
    return row_off, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def _mst_rows(torch, dev, d_matrix, n, row_stride, row_lo, row_hi):
    """The minimum spanning forest of the entries of rows [row_lo, row_hi) of a device distance matrix, built there: (u, v, dist)
    as host arrays, ascending (d, u, v)."""
    room = max(n - 1, 1)
    u = torch.zeros(room, dtype=torch.int32, device="cuda")
    v = torch.zeros(room, dtype=torch.int32, device="cuda")
    dist = torch.zeros(room, dtype=torch.int32, device="cuda")
    k, _ = dev.mst_dev(d_matrix, n, row_stride, row_lo, row_hi, u.data_ptr(), v.data_ptr(), dist.data_ptr())
    return u[:k].cpu().numpy().view(np.uint32), v[:k].cpu().numpy().view(np.uint32), dist[:k].cpu().numpy()


def linkage_on_rank_0(torch, dev, comm, bands, dmat, full, n, kind):
    """The complete- or average-linkage tree of the sorted samples, on rank 0 (None elsewhere): from the device matrix when this
    is the only rank, else from the complete matrix rank 0 has gathered for the tables.  The rounds contract one working matrix,
    which is not distributed over the ranks."""
    if comm.rank != 0:
        return None
    if comm.dist and n:
        return dev.linkage_of_matrix(full, kind)
    m = max(n - 1, 1)
    words = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(4)]
    num = torch.zeros(m, dtype=torch.int64, device="cuda")
    k, _ = dev.linkage_dev(dmat.data_ptr(), n, max(bands.n_padded, 1), kind, *([w.data_ptr() for w in words] + [num.data_ptr()]))
    return tuple(w[:k].cpu().numpy().view(np.uint32) for w in words) + (num[:k].cpu().numpy().view(np.uint64),)


def nj_on_rank_0(torch, dev, comm, bands, dmat, full, n):
    """The neighbour-joining tree of the sorted samples, on rank 0 (None elsewhere), as Device.nj gives it: from the device matrix
    when this is the only rank, else from the complete matrix rank 0 has gathered for the tables — exactly where
    linkage_on_rank_0 gets its matrix.  The rounds work on one matrix, which is not distributed over the ranks."""
    if comm.rank != 0:
        return None
    if comm.dist and n:
        return dev.nj_of_matrix(full)
    m = max(n - 3, 1)
    a, b = (torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(2))
    la, lb = (torch.zeros(m, dtype=torch.int64, device="cuda") for _ in range(2))
    k, star, star_len = dev.nj_dev(dmat.data_ptr(), n, max(bands.n_padded, 1), a.data_ptr(), b.data_ptr(), la.data_ptr(), lb.data_ptr())
    return a[:k].cpu().numpy().view(np.uint32), b[:k].cpu().numpy().view(np.uint32), la[:k].cpu().numpy(), lb[:k].cpu().numpy(), star, star_len


def mst_over_ranks(torch, dev, comm, bands, dmat, band, n):
    """The minimum spanning tree of the whole n x n distance matrix as (u, v, dist) on rank 0, None on the others.  With one rank:
    from `dmat` (pitch bands.n_padded, n columns: the zero padding is never an edge).  With several: each rank builds the forest of
    the complete rows of its band (as close_rows_over_ranks addresses them; an empty band gives no edges), the forests are
    gathered, and rank 0 merges them with Kruskal in the same edge order.  The merge is exact: an edge outside the forest of its
    own band is the largest edge of a cycle of that band, hence of a cycle of the whole graph."""
    if band is not None:
        blo, bhi = bands.band_rows(comm.rank)
        parts = comm.gather_objects(_mst_rows(torch, dev, band.data_ptr() - blo * bands.n_padded * 4, n, bands.n_padded, blo, bhi))
    else:
        parts = [_mst_rows(torch, dev, dmat.data_ptr(), n, max(bands.n_padded, 1), 0, n)]
    if comm.rank != 0:
        return None
    if len(parts) == 1:
        return parts[0]
    return dmod.mst_of_edges(n, *(np.concatenate([p[k] for p in parts]) for k in range(3)))


def _pair_sites_of_packed(torch, dev, packed, n, n_sites, a, b, expect):
    """The differing sites of the pairs (a[p], b[p]) of rows of a device packed matrix (a torch tensor), found there: (pair_off,
    site, bases) as host arrays.  expect: the sum of the pairs' distances — room for the first call; a mismatch costs a second."""
    m = len(a)
    if m == 0 or n == 0:
        return np.zeros(m + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    d_a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint32).view(np.int32)).cuda()
    pair_off = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    capacity = max(int(expect), 1)
    while True:
        site = torch.zeros(capacity, dtype=torch.int32, device="cuda")
        bases = torch.zeros(capacity, dtype=torch.uint8, device="cuda")
        total = dev.pair_sites_dev(packed.data_ptr(), n, n_sites, d_a.data_ptr(), d_b.data_ptr(), m, capacity, pair_off.data_ptr(), site.data_ptr(), bases.data_ptr())
        if total <= capacity:
            break
        capacity = total
    return pair_off.cpu().numpy().view(np.uint64), site[:total].cpu().numpy().view(np.uint32), bases[:total].cpu().numpy()


def stage_matrices_and_distances(job):
    """Collectives interleaved with file output; the output runs under ``job.guard`` so that a rank whose disk is full still takes
    part in every collective and the failure surfaces at the agreement after the stage."""
    torch, comm, sharding, dev = job.torch, job.comm, job.sharding, job.dev
    rank, world, n_total, samples, mine, lo, hi = job.rank, job.world, job.n_total, job.samples, job.mine, job.lo, job.hi
    callable_, outputs, fl = job.callable_, job.outputs, job.flows
    n_local = fl.n_local
    t0 = time.perf_counter()
    # which samples of the whole job have a consensus row (gathered: small)
    ref_seqs = [None]
    ok_local = np.zeros(hi - lo, dtype=bool)
    for k, s in enumerate(callable_):
        ok_local[s.index - lo] = bool(job.row_ok[k])
    ok_all = np.concatenate(comm.gather_objects(ok_local)) if n_total else np.zeros(0, bool)
    local_row_of = {s.index: k for k, s in enumerate(callable_)}
    for flow, rows, Sx, excluded, snpma, pairs, matrix in ((1, job.rows1, fl.S1, job.excluded1, "snpma", "pairs", "matrix"),
                                                          (2, job.rows2, fl.S2, job.excluded2, "snpma_p", "pairs_p", "matrix_p")):
        # snp_matrix (snp_matrix.py:79-119): the samples of the step's filtered list, sorted-dir order, that have a consensus file
        member = ok_all & ~excluded
        if not member.any():                                 # every rank sees the same flags: all leave, rank 0 says why
            if rank == 0:
                utils.global_error("Error: all %d consensus fasta files were missing or empty." % int((~excluded).sum()))
            sys.exit(100)
        chunks = []
        for s in mine:
            if member[s.index]:
                k = local_row_of[s.index]
                chunks.append(_fasta_bytes(s.name, rows[k, :Sx].cpu().numpy() if Sx else np.zeros(0, np.uint8)))
        blob = b"".join(chunks)
        sizes = comm.gather_objects(len(blob))
        with job.guard() as go:
            if go and rank == 0:
                with open(outputs[snpma], "wb") as f:
                    f.truncate(sum(sizes))
        comm.barrier()
        with job.guard() as go:
            if go:
                with open(outputs[snpma], "r+b") as f:
                    f.seek(sum(sizes[:rank]))
                    f.write(blob)
        # distance (distance.py:76-114): ids = sorted names, equal names keep the last record of the file
        last = {}
        for i in np.flatnonzero(member):
            last[samples[i].name] = i
        ids = sorted(last)
        order = np.asarray([last[i] for i in ids], dtype=np.int64)
        n = len(ids)
        row_bytes = dev.packed_row_bytes(Sx)
        per = (n_total + world - 1) // world if n_total else 0
        packed_local = torch.zeros((max(hi - lo, 1), row_bytes), dtype=torch.uint8, device="cuda")
        if n_local and Sx:
            tmp = torch.zeros((n_local, row_bytes), dtype=torch.uint8, device="cuda")
            dev.pack_matrix_dev(rows.data_ptr(), n_local, Sx, rows.shape[1], tmp.data_ptr())
            # (row k of the pack belongs to the k-th callable sample: to its place in this rank's block — a library kernel, no ATen indexing)
            idx = torch.from_numpy(np.asarray([s.index - lo for s in callable_], dtype=np.uint32)).cuda()
            dev.rows_copy_dev(tmp.data_ptr(), row_bytes, packed_local.data_ptr(), row_bytes, n_local, row_bytes, d_dst_index=idx.data_ptr())
        packed_all = torch.zeros((max(world * per, 1), row_bytes), dtype=torch.uint8, device="cuda")
        sharding.all_gather_rows_into(packed_local[:hi - lo], n_total, packed_all)
        bands = sharding.RowBands(n, world)
        packed_sorted = torch.zeros((max(bands.n_padded, 1), row_bytes), dtype=torch.uint8, device="cuda")
        if n and row_bytes:
            d_order = torch.from_numpy(order.astype(np.uint32)).cuda()
            dev.rows_copy_dev(packed_all.data_ptr(), row_bytes, packed_sorted.data_ptr(), row_bytes, n, row_bytes, d_src_index=d_order.data_ptr())
        dmat = torch.zeros((max(bands.n_padded, 1), max(bands.n_padded, 1)), dtype=torch.int32, device="cuda")
        if n and Sx:
            dev.distance_packed_dev(packed_sorted.data_ptr(), bands.n_padded, Sx, dmat.data_ptr(), rank, world)
        if comm.dist and n:
            band = bands.exchange(dmat, rank)                # the complete rows of this rank's band
            blo, bhi = bands.band_rows(rank)
            pieces = comm.gather_objects(band[:bhi - blo, :n].cpu().numpy())
            full = np.concatenate(pieces, axis=0) if rank == 0 else None
        else:
            full = dmat[:n, :n].cpu().numpy()
        csr = None
        if job.close_pairs is not None or job.cluster_thresholds:
            # every rank thresholds the complete rows it holds on the device; the pieces that travel are the pairs within the widest threshold
            widest = max(([job.close_pairs] if job.close_pairs is not None else []) + job.cluster_thresholds)
            csr = close_rows_over_ranks(torch, dev, comm, bands, dmat, band if (comm.dist and n) else None, n, widest)
        with job.guard() as go:
            if go and rank == 0 and csr is not None:
                sfx = "" if flow == 1 else "_p"
                dmod.write_pairs_and_clusters(dev, ids, csr[0], csr[1], csr[2], outputs["close" + sfx] if job.close_pairs is not None else None, job.close_pairs,
                                              outputs["clusters" + sfx] if job.cluster_thresholds else None, job.cluster_thresholds)
        tree = mst_over_ranks(torch, dev, comm, bands, dmat, band if (comm.dist and n) else None, n) if job.mst else None
        with job.guard() as go:
            if go and rank == 0 and tree is not None:
                sfx = "" if flow == 1 else "_p"
                dmod.write_mst(outputs["mst" + sfx], ids, *tree)
                dmod.write_dendrogram(outputs["dendrogram" + sfx], ids, *tree)
        with job.guard() as go:
            if go and job.linkage:
                merges = linkage_on_rank_0(torch, dev, comm, bands, dmat, full, n, job.linkage)
                if rank == 0:
                    sfx = "" if flow == 1 else "_p"
                    dmod.write_linkage_outputs(ids, job.linkage, merges, outputs["linkage" + sfx], outputs["linkage_nwk" + sfx],
                                               outputs["linkage_clusters" + sfx] if job.cluster_thresholds else None, job.cluster_thresholds)
        with job.guard() as go:
            if go and job.nj:
                nj_tree = nj_on_rank_0(torch, dev, comm, bands, dmat, full, n)
                if rank == 0:
                    dmod.write_nj(outputs["nj" if flow == 1 else "nj_p"], ids, *nj_tree)
        with job.guard() as go:
            # every rank holds packed_sorted after the all-gather: rank 0 asks it for the sites behind the gathered pairs and edges
            if go and rank == 0 and job.pair_sites:
                sfx = "" if flow == 1 else "_p"
                snp_list = utils.read_snp_position_list(outputs["snplist" + sfx])
                if len(snp_list) != Sx:
                    raise RuntimeError("%s lists %d sites, the matrix has %d columns" % (outputs["snplist" + sfx], len(snp_list), Sx))
                if job.close_pairs is not None:
                    a, b, d = dmod.pairs_of_csr(csr[0], csr[1], csr[2], job.close_pairs)
                    got = _pair_sites_of_packed(torch, dev, packed_sorted, n, Sx, a, b, int(d.sum(dtype=np.int64)))
                    dmod.write_pair_sites(outputs["close_sites" + sfx], ids, a, b, *got, snp_list=snp_list)
                if tree is not None:
                    got = _pair_sites_of_packed(torch, dev, packed_sorted, n, Sx, tree[0], tree[1], int(np.asarray(tree[2]).sum(dtype=np.int64)))
                    dmod.write_pair_sites(outputs["mst_sites" + sfx], ids, tree[0], tree[1], *got, snp_list=snp_list)
        with job.guard() as go:
            if go and rank == 0:
                dmod.write_pairwise(outputs[pairs], ids, full)
                dmod.write_matrix(outputs[matrix], ids, full)
                if ref_seqs[0] is None:
                    ref_seqs[0] = snp_reference.read_fasta_sequences(job.ref_path)
                snp_reference.write_reference_snp_file(job.ref_path, outputs["snplist" if flow == 1 else "snplist_p"],
                                                       outputs["refsnp" if flow == 1 else "refsnp_p"], match_dict=ref_seqs[0])
    comm.barrier()
    job.lap("4 matrices + distances", t0)


# ==================================== stage 5: the VCF files the per-sample command writes ====================================
def stage_leftover_vcfs(job):
    """Samples whose pileup repeats a listed position get consensus.vcf rows for EVERY matching line from the per-sample command
    (call_consensus.py:178-180); its consensus.fasta is the same bytes the job wrote.  With --vcfAllPos: every sample."""
    vcf_again = job.vcf_again
    if job.vcf_all_pos:
        vcf_again = [s for k, s in enumerate(job.callable_) if job.row_ok[k]]
    if not vcf_again:
        return
    from . import call_consensus as cc_step
    outputs, ref_path = job.outputs, job.ref_path
    quiet = argparse.Namespace(verbose=0)
    utils.set_logging_verbosity(quiet)
    process_device, devmod._default = devmod._default, job.dev   # (the command's "process-wide device" is this job's context)
    try:
        for s in vcf_again:
            if not s.ok:
                continue
            try:
                for snplist, suffix, more in ((outputs["snplist"], "", []),
                                              (outputs["snplist_p"], "_preserved", ["-e", os.path.join(s.dir, "var.flt_removed.vcf")])):
                    cc_step.call_consensus(_step_args("call_consensus", ["-f", "-l", snplist, "-o", os.path.join(s.dir, "consensus%s.fasta" % suffix),
                                                                         "--vcfRefName", os.path.basename(ref_path), "--vcfFileName", "consensus%s.vcf" % suffix]
                                                      + more + [s.pileup], job.cc_extra))
            except (Exception, SystemExit) as e:             # noqa: B902 — reported as this sample's error below
                s.fail("Error: call_consensus failed for sample %s: %s: %s" % (s.name, type(e).__name__, e))
    finally:
        devmod._default = process_device
        utils.set_logging_verbosity(job.args)


def stage_collect_metrics(job):
    """--collectMetrics: the metrics file of every sample of this rank (collect_metrics.run_batch), with the depth sums and gap
    counts the job holds as `known` and the VCF files it has just written counted in one stream on the job's device.  The table
    is written by rank 0 when every rank has got here (hot_path_batch)."""
    if not job.collect_metrics:
        return
    from . import collect_metrics as cm
    t0 = time.perf_counter()
    options = cm.Options.from_args(_step_args("collect_metrics_batch", [job.dirs_file, job.ref_path], job.cm_extra))
    job.metrics_options = options
    job.dev.sync()
    job.metrics_done = cm.run_batch([s.dir for s in job.mine], job.ref_path, options, devices=[job.dev], known=job.metrics_known,
                                    report_errors=False)
    for s, message in ((s, job.metrics_done["errors"].get(s.dir)) for s in job.mine):
        if message and s.ok:
            s.fail(message)
    job.lap("collect_metrics", t0)


STAGES = (stage_ingest_and_sites, stage_site_union_and_regions, stage_consensus, stage_matrices_and_distances, stage_leftover_vcfs,
          stage_collect_metrics)


def _job_stats(job):
    st = job.store.stats() if job.store is not None else L.PileupsStats()
    fl = job.flows
    if job.pileup_route == "stream":                         # nothing was ingested: the figures are those of the consensus stage's streamed calls
        st.file_bytes, st.n_files, st.n_readers = job.stream_stats["file_bytes"], job.stream_stats["files"], job.stream_stats["readers"]
    done = getattr(job, "metrics_done", None)
    return {"collect_metrics": {k: v for k, v in done.items() if k != "errors"} if done else None,
            "h2d_bytes": int(st.h2d_bytes) + job.h2d_extra, "file_bytes": int(st.file_bytes), "resident_files": int(st.n_resident),
            "files": int(st.n_files), "seconds": time.perf_counter() - job.t_start, "site_calling": job.site_calling,
            "pileup_route": job.pileup_route, "vcf_again": len(getattr(job, "vcf_again", ())),
            "ingest": {"seconds": st.seconds, "allocating": st.seconds_allocating, "waiting_for_readers": st.seconds_waiting_for_readers,
                       "waiting_for_device": st.seconds_waiting_for_device, "reader_seconds_reading": st.reader_seconds_reading,
                       "reader_seconds_waiting": st.reader_seconds_waiting, "preparing": st.seconds_preparing},
            "phases": job.timings, "call_passes": dict(job.call_passes), "sites": fl.S1, "sites_preserved": fl.S2, "samples": job.hi - job.lo,
            "readers": int(st.n_readers), "usable_cores": job.cpu["usable_cpus"], "local_world": job.cpu["local_ranks"], "cpu_budget": job.cpu}


def hot_path_batch(args):
    """Entry point of ``cfsan_snp_pipeline hot_path_batch`` (an extension of this build; see the module docstring).

    ``hot_path_batch.last_stats`` holds this rank's figures of the last run (``_job_stats``).  Its key ``call_passes`` is a dict
    over ``Device.CALL_PASS_NAMES`` (lanes128, lanes256, lanes512, wave): how many pileup lines of the job's consensus step each
    call kernel took, summed over the groups of samples whose call was one launch; ``groups_not_counted``, when present, is the
    number of groups that took several launches and are left out.  Lines under ``wave`` left the one-lane-per-site path: they
    are longer than 512 bytes (a sample deeper than about 240x) or malformed.  ``-v 2`` logs the same figures per group.
    ``pileup_route`` is the route this rank took (resident / stream, ``auto`` resolved); on route stream ``resident_files`` is 0
    and ``h2d_bytes`` / ``file_bytes`` / ``files`` count what the consensus stage streamed.  ``vcf_again`` is the number of
    samples whose VCF files the per-sample command wrote at the end (repeated positions, spill records of a mixed group)."""
    utils.print_log_header(classpath=True)
    utils.print_arguments(args)
    if getattr(args, "mergeVcfs", False) and args.noConsensusVcf:
        utils.global_error("Error: --mergeVcfs merges the consensus.vcf files of the job: it cannot be combined with --noConsensusVcf.")
    if getattr(args, "mergeVcfs", False):
        from . import merge_vcfs as mv
        mv.merge_device_bytes(getattr(args, "mergeDeviceBytes", None))      # (a value that is no count ends the job before it starts)
    comm = _Comm()
    job = _Job(args, comm)
    if not args.forceFlag and job.is_fresh():
        verbose_print("All outputs of the hot path have already been freshly built.  Use the -f option to force a rebuild.")
        comm.close()
        return
    try:
        job.open_device()
        for stage in STAGES:
            job.run_stage(stage)
        stats = _job_stats(job)
        hot_path_batch.last_stats = stats
        if os.environ.get("SNPGPU_HOT_PATH_STATS"):             # a directory: every rank leaves its figures there (tests, bench tooling)
            import json
            with open(os.path.join(os.environ["SNPGPU_HOT_PATH_STATS"], "rank%d.json" % job.rank), "w") as f:
                json.dump(stats, f)
        verbose_print("# hot_path_batch rank %d: %d samples, %d pileup bytes, %d bytes copied to the device (%d files resident), %.3f s"
                      % (job.rank, job.hi - job.lo, stats["file_bytes"], stats["h2d_bytes"], stats["resident_files"], stats["seconds"]))
        for k in sorted(job.timings):
            verbose_print("#   %-34s %.3f s" % (k, job.timings[k]))
    finally:
        job.close_device()
    # ---- per-sample errors: reported the way the batch subcommands do ----------------------------------------------------
    errs = [s.error for s in job.mine if not s.ok]
    all_errs = comm.gather_objects(errs)
    failed = sum(len(e) for e in all_errs)
    if job.collect_metrics and job.rank == 0 and getattr(job, "metrics_options", None) is not None:    # (every rank's metrics files are written: the gather above)
        from . import collect_metrics as cm
        merged = args.mergedMetricsFile or os.path.join(job.work_dir, "metrics.tsv")
        cm.combine(job.unsorted_dirs, job.metrics_options.metricsFile, merged, bool(getattr(args, "spaceHeadings", False)))
    comm.close()                                             # (before anything that may end the process: sample_error exits when StopOnSampleError says so)
    for msg in errs:
        utils.sample_error(msg, continue_possible=True)
    if failed:
        verbose_print("%d of %d samples failed." % (failed, job.n_total))
        if not errs and utils._stop_on_sample_error():       # a peer's sample failed: leave with the code it leaves with
            sys.exit(100)
    # merge_vcfs may end the process (a sample without its VCF, a line outside the rule, a missing tool): it runs after the group
    # is closed and this rank's sample errors are reported; every rank's consensus*.vcf files are written (the gather above)
    if getattr(args, "mergeVcfs", False) and job.rank == 0:
        _merge_vcfs_stage(job)


hot_path_batch.last_stats = None


def _merge_vcfs_stage(job):
    """--mergeVcfs: snpma.vcf and snpma_preserved.vcf in the work directory, as run.py:755-766 asks merge_vcfs for them: from the
    files the job has just written, for the samples of each flow's filtered list, through the subcommand's own library call."""
    from . import merge_vcfs as mv
    t0 = time.perf_counter()
    routes = {}
    for listing, name, out in ((job.filtered1, "consensus.vcf", "snpma.vcf"), (job.filtered2, "consensus_preserved.vcf", "snpma_preserved.vcf")):
        with open(listing, "r") as f:
            dirs = [d for d in (line.rstrip() for line in f) if d]
        routes[out] = mv.merge_sample_dirs(dirs, name, os.path.join(job.work_dir, out), force=True, merger=getattr(job.args, "vcfMerger", None),
                                           device_bytes=getattr(job.args, "mergeDeviceBytes", None))
    job.timings["merge_vcfs"] = time.perf_counter() - t0
    if hot_path_batch.last_stats is not None:
        hot_path_batch.last_stats["merge_vcfs"] = routes
    verbose_print("#   %-34s %.3f s" % ("merge_vcfs", job.timings["merge_vcfs"]))


def _fasta_bytes(name, seq):
    """The bytes of a consensus FASTA file (utils.write_fasta_record): what snp_matrix copies into snpma.fasta."""
    n = len(seq)
    head = (">%s\n" % name).encode("utf-8")
    if n == 0:
        return head
    full, tail = divmod(n, 60)
    body = np.full((full + (1 if tail else 0), 61), 0x0A, dtype=np.uint8)
    if full:
        body[:full, :60] = seq[:full * 60].reshape(full, 60)
    out = body[:full].tobytes()
    if tail:
        out += seq[full * 60:].tobytes() + b"\n"
    return head + out


def _call_scattered(dev, ss, prm, res_idx, ptrs, sizes, d_base, d_filt, d_status, d_counts, d_line, S, want_vcf, torch, want_depth_sum=False):
    """A group in which only some samples are resident: they are called into temporary arrays and scattered to their rows."""
    m = len(res_idx)
    tb = torch.empty((m, S), dtype=torch.uint8, device="cuda")
    tf = torch.empty((m, S), dtype=torch.uint8, device="cuda")
    tl = torch.zeros((m, S), dtype=torch.int64, device="cuda")
    ts = torch.empty((m, 4), dtype=torch.int64, device="cuda")
    tc = torch.empty((m, S, 128), dtype=torch.uint8, device="cuda") if want_vcf else None
    dev.call_consensus_many_dev(ss, ptrs, sizes, prm, tb.data_ptr(), tf.data_ptr(), ts.data_ptr(), d_counts=tc.data_ptr() if want_vcf else 0,
                                d_line_off=tl.data_ptr(), want_depth_sum=want_depth_sum)
    # to their rows through the library's row copy (no ATen index kernels between the job's own: VERDICT r5 #7)
    idx = torch.from_numpy(np.asarray(res_idx, dtype=np.uint32)).cuda()
    for src, dst, item in ((tb, d_base, 1), (tf, d_filt, 1), (tl, d_line, 8), (ts, d_status, 8)) + (((tc, d_counts, 128),) if want_vcf else ()):
        width = 4 if dst is d_status else S                       # elements of a row that are copied
        dev.rows_copy_dev(src.data_ptr(), src.stride(0) * src.element_size(), dst.data_ptr(), dst.stride(0) * dst.element_size(), m, width * item,
                          d_dst_index=idx.data_ptr())


def add_arguments(sub):
    sub.add_argument(dest="sampleDirsFile", type=str, help="Relative or absolute path to file containing a list of directories -- one per sample")
    sub.add_argument(dest="referenceFile", type=str, help="Relative or absolute path to the reference fasta file")
    sub.add_argument("-f", "--force", dest="forceFlag", action="store_true", help="Force processing even when result files already exist and are newer than inputs")
    sub.add_argument("--workDir", dest="workDir", type=str, default=None, metavar="DIR", help="Directory of the top-level output files (default: the directory of sampleDirsFile)")
    sub.add_argument("--pileupName", dest="pileupName", type=str, default="reads.all.pileup", metavar="NAME", help="File name of the genome-wide pileup file in each sample directory.")
    sub.add_argument("--siteCalling", dest="siteCalling", type=str, default=None, choices=cs.SITE_CALLING_MODES, metavar="MODE",
                     help="Who writes var.flt.vcf: varscan (the VarScan jar on CLASSPATH, as the reference), device (this build's restatement; parity unpinned), "
                          "existing (nobody: the files are inputs and stay byte for byte), auto (varscan when a jar is on CLASSPATH, else device).  Default: $SNPGPU_SITE_CALLING, else auto")
    for name, env in (("filterRegionsExtraParams", "FilterRegions_ExtraParams"), ("mergeSitesExtraParams", "MergeSites_ExtraParams"),
                      ("callConsensusExtraParams", "CallConsensus_ExtraParams"), ("varscanExtraParams", "VarscanMpileup2snp_ExtraParams")):
        sub.add_argument("--" + name, dest=name, type=str, default=None, metavar="STRING",
                         help="Options of that step, as the configuration file gives them (default: the environment variable %s)" % env)
    sub.add_argument("--collectMetrics", dest="collectMetrics", action="store_true", help="At the end of the job write every sample's metrics file and the merged table (collect_metrics_batch), from the depth sums and gap counts the job holds: no pileup is read a second time")
    sub.add_argument("--collectMetricsExtraParams", dest="collectMetricsExtraParams", type=str, default=None, metavar="STRING", help="Options of collect_metrics, as the configuration file gives them (default: the environment variable CollectMetrics_ExtraParams)")
    sub.add_argument("--mergedMetricsFile", dest="mergedMetricsFile", type=str, default=None, metavar="PATH", help="With --collectMetrics: the merged metrics table (default: metrics.tsv in the work directory)")
    sub.add_argument("--mergeVcfs", dest="mergeVcfs", action="store_true", help="At the end of the job write snpma.vcf and snpma_preserved.vcf (merge_vcfs) into the work directory, from the consensus.vcf / consensus_preserved.vcf files the job has just written; not with --noConsensusVcf")
    sub.add_argument("--vcfMerger", dest="vcfMerger", type=str, default=None, choices=("bcftools", "device", "auto"), metavar="MODE", help="With --mergeVcfs: who merges, as merge_vcfs --vcfMerger (default: $SNPGPU_VCF_MERGER, else auto)")
    sub.add_argument("--mergeDeviceBytes", dest="mergeDeviceBytes", type=str, default=argparse.SUPPRESS, metavar="INT", help="With --mergeVcfs: the device memory the device route may allocate, as merge_vcfs --mergeDeviceBytes (default: $SNPGPU_MERGE_DEVICE_BYTES, else 0 = what is free, less a reserve)")
    sub.add_argument("--closePairs", dest="closePairs", type=int, default=None, metavar="INT", help="Also write snp_distance_close_pairs.tsv and snp_distance_close_pairs_preserved.tsv into the work directory: the rows of the pairwise files whose distance is at most INT, thresholded on the device (as distance --amdClosePairs --amdMaxPairDistance)")
    sub.add_argument("--clusters", dest="clusters", type=int, nargs="+", default=None, metavar="INT", help="Also write snp_clusters.tsv and snp_clusters_preserved.tsv into the work directory: every sample's single-linkage cluster number at each of the SNP thresholds (as distance --amdClusters --amdClusterThresholds)")
    sub.add_argument("--mst", dest="mst", action="store_true", help="Also write snp_mst.tsv, snp_mst_preserved.tsv, snp_dendrogram.nwk and snp_dendrogram_preserved.nwk into the work directory: the minimum spanning tree of the samples and their single-linkage dendrogram, built on the device (as distance --amdMst --amdDendrogram)")
    sub.add_argument("--linkage", dest="linkage", type=str, choices=["complete", "average"], default=None, help="Also write snp_linkage.tsv, snp_linkage_preserved.tsv, snp_linkage.nwk and snp_linkage_preserved.nwk into the work directory: the merges and the dendrogram of the complete- or average-linkage tree of the samples (as distance --amdLinkage --amdLinkageMerges --amdLinkageDendrogram), and with --clusters snp_linkage_clusters.tsv and snp_linkage_clusters_preserved.tsv: the tree cut at each of the thresholds (as --amdLinkageClusters).  Built on the device of rank 0 from the complete matrix it gathers for the tables; the linkage itself is not distributed over the ranks")
    sub.add_argument("--nj", dest="nj", action="store_true", help="Also write snp_nj.nwk and snp_nj_preserved.nwk into the work directory: the neighbour-joining tree of the samples as one Newick line with branch lengths in SNPs (as distance --amdNj).  Built on the device of rank 0 from the matrix the linkage tree would be built from; the rounds are not distributed over the ranks")
    sub.add_argument("--pairSites", dest="pairSites", action="store_true", help="With --closePairs: also write snp_close_pair_sites.tsv and snp_close_pair_sites_preserved.tsv, with --mst: snp_mst_sites.tsv and snp_mst_sites_preserved.tsv, into the work directory: the sites (Chrom and Pos of the flow's snplist) at which the two samples of every close pair i < j / of every tree edge differ, and their bases, found on the device (as distance --amdClosePairSites / --amdMstSites --amdSnpList)")
    sub.add_argument("--noConsensusVcf", dest="noConsensusVcf", action="store_true", help="Do not write consensus.vcf / consensus_preserved.vcf")
    sub.add_argument("--residentBytes", dest="residentBytes", type=int, default=0, metavar="INT", help="Device memory for resident pileups (0 = what is free, less 24 GiB); files past it are streamed twice in site calling mode device only: in modes existing and varscan --pileupRoute auto streams every pileup once instead")
    sub.add_argument("--pileupRoute", dest="pileupRoute", type=str, default=None, choices=PILEUP_ROUTES, metavar="ROUTE",
                     help="How the pileups reach the consensus scan: resident (kept in device memory between site calling and the scan; files past --residentBytes are read a second time), "
                          "stream (nothing is kept: the site lists are made first and each pileup is scanned and called as it lands, once, at any size; site calling modes existing and varscan only), "
                          "auto (stream where the mode allows it and this rank's pileup bytes exceed the resident budget, else resident).  Default: $SNPGPU_PILEUP_ROUTE, else auto")
    sub.add_argument("--groupBytes", dest="groupBytes", type=int, default=0, metavar="INT", help="Host bytes of per-site results per group of samples (default 1 GiB)")
    sub.add_argument("--writerThreads", dest="writerThreads", type=int, default=0, metavar="INT", help="Host threads that write the consensus files (0 = up to 64)")
