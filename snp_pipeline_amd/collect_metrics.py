"""``cfsan_snp_pipeline collect_metrics_batch`` — an extension of this build: every sample's metrics file and the merged
metrics.tsv in one job.

The reference starts one ``collect_metrics`` process per sample (run.py) and then ``combine_metrics``.  Per sample, Python
reads the whole pileup again to sum its depth column (collect_metrics.py:325-340), parses four VCF files with PyVCF to count
SNPs (:61-106) and two FASTA files to count gaps (:109-128).  Here the depth sums of all stale pileups come out of ONE
stream through the pileup scan, the SNP counts of all stale VCF files out of ONE stream through the count kernel
(csrc/vcf_count.hip), and the rest is host work on a pool sized by the CPU budget.

  count_snps_line / count_snps_text   the counting rule as plain text processing (what the kernel and the host must agree on)
  count_snps_files                    device counts + host evaluation of the lines the kernel leaves alone
  collect_one                         the twenty values of collect_metrics.py:467-487 for one sample
  combine                             the table of combine_metrics.py:67-113
  run_batch / collect_metrics_batch   the job
"""
from __future__ import print_function

import glob
import gzip
import os
import re
import shutil
import subprocess
import sys

from . import utils
from .utils import verbose_print

LINE_WINDOW = 4096                  # SNPGPU_VCF_LINE_WINDOW: a line of this many bytes or more is left to the host
SNP_LETTERS = (b"A", b"C", b"G", b"T", b"N")
UNUSUAL_CAPACITY = 64

METRIC_NAMES = ("sample", "fastqFileList", "fastqFileSize", "machine", "flowcell", "numberReads", "numberDupReads", "percentReadsMapped",
                "percentProperPair", "aveInsertSize", "avePileupDepth", "phase1Snps", "phase1SnpsPreserved", "snps", "snpsPreserved",
                "missingPos", "missingPosPreserved", "excludedSample", "excludedSamplePreserved", "errorList")
QUOTED_METRICS = ("sample", "fastqFileList", "errorList")
COLUMN_HEADINGS = ("Sample", "Fastq Files", "Fastq File Size", "Machine", "Flowcell", "Number of Reads", "Duplicate Reads", "Percent of Reads Mapped",
                   "Percent Proper Pair", "Average Insert Size", "Average Pileup Depth", "Phase1 SNPs", "Phase1 Preserved SNPs", "Phase2 SNPs",
                   "Phase2 Preserved SNPs", "Missing SNP Matrix Positions", "Missing Preserved SNP Matrix Positions", "Excluded Sample",
                   "Excluded Preserved Sample", "Warnings and Errors")


# ---- the counting rule -------------------------------------------------------------------------------------------------------
def _sample_counts(ref, alts, names, sample):
    """One sample column under the rule of collect_metrics.py:88-105: True when it is one SNP."""
    values = dict(reversed(list(zip(names, sample.split(b":")))))    # (a name that comes twice: its first place, as the kernel)
    gt = values.get(b"GT")
    if gt is None:
        return False
    tokens = re.split(b"[/|]", gt)
    if b"." in tokens:
        return False
    if not all(t.isdigit() for t in tokens):                 # (PyVCF stops at such a row; nothing pins what to do instead)
        return False
    index = [int(t) for t in tokens]
    alleles = [ref] + alts
    if any(i >= len(alleles) for i in index) or not any(index):
        return False
    if not any(alleles[i] in SNP_LETTERS for i in index):    # a spanning deletion (*) is no SNP
        return False
    return b"FT" not in names or values.get(b"FT") == b"PASS"   # (an FT the sample column leaves out is no PASS)


def count_snps_line(line):
    """The number of SNPs a data line (bytes, no terminator) stands for: one per sample column that passes."""
    cols = line.split(b"\t")
    if len(cols) < 10:
        return 0
    names = cols[8].split(b":")
    alts = cols[4].split(b",")
    return sum(1 for sample in cols[9:] if _sample_counts(cols[3], alts, names, sample))


def is_unusual_line(line, raw=None):
    """A data line outside the grammar the kernel judges (include/snpgpu.h): the kernel reports it, the host counts it.
    raw: its length in the file without the LF (a CR counts: it is inside the kernel's window)."""
    if (len(line) if raw is None else raw) >= LINE_WINDOW:
        return True
    cols = line.split(b"\t")
    if len(cols) != 10:
        return True
    names, values = cols[8].split(b":"), cols[9].split(b":")
    if len(names) != len(values) or b"GT" not in names:
        return True
    n_alleles = 2 + cols[4].count(b",")
    for t in re.split(b"[/|]", values[names.index(b"GT")]):
        if t != b"." and (not t.isdigit() or int(t) >= n_alleles):
            return True
    return False


def data_lines(data):
    """The data lines of VCF text (bytes): split at LF, a CR in front of it dropped, empty lines and '#' lines left out.
    Yields (byte offset of the line, line, raw length)."""
    at = 0
    n = len(data)
    while at < n:
        end = data.find(b"\n", at)
        if end < 0:
            end = n
        raw = end - at
        line = data[at:end - 1] if raw and data[end - 1:end] == b"\r" else data[at:end]
        if line and not line.startswith(b"#"):
            yield at, line, raw
        at = end + 1


def count_snps_text(data):
    """(SNPs, data lines, unusual lines, SNPs among the usual lines) of VCF text: the whole rule on the host."""
    snps = n_data = unusual = usual_snps = 0
    for _, line, raw in data_lines(data):
        n_data += 1
        k = count_snps_line(line)
        snps += k
        if is_unusual_line(line, raw):
            unusual += 1
        else:
            usual_snps += k
    return snps, n_data, unusual, usual_snps


def count_snps_python(path):
    with open(path, "rb") as f:
        return count_snps_text(f.read())[0]


def _line_ending_at(f, end):
    """The line of the open file whose terminator is the byte at offset `end`, without it (read backwards in blocks)."""
    parts, at = [], end
    while at > 0:
        lo = max(0, at - 65536)
        f.seek(lo)
        block = f.read(at - lo)
        cut = block.rfind(b"\n")
        if cut >= 0:
            parts.append(block[cut + 1:])
            break
        parts.append(block)
        at = lo
    return b"".join(reversed(parts))


def count_snps_files(dev, paths, capacity=UNUSUAL_CAPACITY):
    """The SNP count of every VCF file of `paths` (count_vcf_file_snps of the reference): the device counts the rows inside
    its grammar in one stream over all files, the host adds the lines the kernel reported as unusual: each of them read at its
    offset (a line longer than the kernel's window is reported by its terminator and read backwards from there; it may be a
    header line, which counts nothing) — or the whole file when there are more of them than `capacity`.  Returns a list of ints;
    an IOError object stands for a file that cannot be read."""
    from . import _lib as L
    out = []
    for path, res in zip(paths, dev.vcf_count_snps_files(paths, capacity)):
        if isinstance(res, Exception):
            out.append(res)
            continue
        snps, _, unusual, offsets, status = res
        if unusual:
            if status & L.VCF_MORE_UNUSUAL:
                snps = count_snps_python(path)
            else:
                with open(path, "rb") as f:
                    for off in offsets:
                        if off >> 63:
                            line = _line_ending_at(f, off & ((1 << 63) - 1))
                        else:
                            f.seek(off)
                            line = f.readline().rstrip(b"\n")
                        line = line[:-1] if line.endswith(b"\r") else line
                        if line and not line.startswith(b"#"):
                            snps += count_snps_line(line)
        out.append(snps)
    return out


# ---- fastq headers (fastq.py:14-56, :185-419 of the reference) ---------------------------------------------------------------
FASTQ_SUFFIXES = ("*.fastq", "*.fastq.gz", "*.fq", "*.fq.gz")
# <flowcell>:<lane>:<tile>:<x>:<y>, ':' or '_' between them; optionally <instrument>:<run>: in front; optionally an SRA / ENA
# run accession and a blank or '_' in front of that
_TAIL = r"([a-zA-Z0-9\-]*)[:_]([0-9]{1,2})[:_][0-9]+[:_][0-9]+[:_][0-9]+"
_ACCESSION = r"[SE]RR[A-Z0-9\-.]+[ _]"
_MACHINE = r"([A-Z][A-Z0-9\-]*)[:_]([0-9]+)[:_]"
_WITHOUT_MACHINE = [re.compile("@" + _TAIL), re.compile("@" + _ACCESSION + _TAIL)]
_WITH_MACHINE = [re.compile("@" + _MACHINE + _TAIL), re.compile("@" + _ACCESSION + _MACHINE + _TAIL)]


def list_fastq_files(directory):
    found = []
    for suffix in FASTQ_SUFFIXES:
        found.extend(glob.glob(os.path.join(directory, suffix)))
    found.sort()
    return found


def parse_seqid_line(line):
    """(instrument or None, flowcell) of the first header line of a fastq file, None when it is no Illumina header."""
    line = line.replace('"', "")
    instrument = None
    for regex in _WITHOUT_MACHINE:
        m = regex.search(line)
        if m:
            flowcell = m.group(1)
            break
    else:
        for regex in _WITH_MACHINE:
            m = regex.search(line)
            if m:
                instrument, flowcell = m.group(1), m.group(3)
                break
        else:
            return None
    parts = flowcell.split("-")
    if not parts[0].strip("0"):                                 # nothing but zeros in front of the '-'
        flowcell = parts[-1]
    return instrument, flowcell


def extract_metadata_tags(fastq_path):
    opener = gzip.open if fastq_path.endswith(".gz") else open
    with opener(fastq_path, "rt") as f:
        return parse_seqid_line(f.readline())


# ---- one sample ------------------------------------------------------------------------------------------------------------------
def read_properties(path):
    """name=value lines as utils.read_properties of the reference reads them (utils.py:384-420, without variables)."""
    props = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("#") or "=" not in line:
                continue
            key, value = line.split("=", 1)
            value = value.strip()
            if value.startswith('"') and value.endswith('"'):
                value = value.strip('"')
            elif value.startswith("'") and value.endswith("'"):
                value = value.strip("'")
            props[key.strip()] = value
    return props


def count_missing_positions(fasta_path, sample_id):
    """Gaps of the record whose id is the sample id, 0 when there is none (collect_metrics.py:109-128)."""
    records = utils.fasta_records_ascii(fasta_path)
    if records is not None:
        for name, seq in records:
            if name == sample_id:
                return seq.count(b"-")
        return 0
    name, n = None, 0
    with open(fasta_path, "r") as f:
        for line in f:
            if line.startswith(">"):
                if name == sample_id:
                    return n
                words = line[1:].split()
                name, n = (words[0] if words else ""), 0
            elif name is not None:
                n += "".join(line.split()).count("-")
    return n if name == sample_id and name is not None else 0


def pileup_depth_sum_python(path):
    """The loop of collect_metrics.py:325-332 (for a pileup the device refuses)."""
    depth_sum = 0
    with open(path) as f:
        for line in f:
            tokens = line.split()
            try:
                depth_sum += int(tokens[3])
            except (ValueError, IndexError):
                pass
    return depth_sum


class Options(object):
    """The options of the reference's collect_metrics parser (cfsan_snp_pipeline.py:478-488), same defaults."""

    def __init__(self, forceFlag=False, metricsFile="metrics", maxSnps=-1, consensusFastaFileName="consensus.fasta",
                 consensusPreservedFastaFileName="consensus_preserved.fasta", consensusVcfFileName="consensus.vcf",
                 consensusPreservedVcfFileName="consensus_preserved.vcf"):
        self.forceFlag = forceFlag
        self.metricsFile = metricsFile
        self.maxSnps = maxSnps
        self.consensusFastaFileName = consensusFastaFileName
        self.consensusPreservedFastaFileName = consensusPreservedFastaFileName
        self.consensusVcfFileName = consensusVcfFileName
        self.consensusPreservedVcfFileName = consensusPreservedVcfFileName

    @classmethod
    def from_args(cls, args):
        return cls(**{k: getattr(args, k) for k in cls().__dict__ if hasattr(args, k)})


def metrics_path(sample_dir, options):
    return os.path.join(sample_dir, options.metricsFile)


def _usable(path):
    return os.path.isfile(path) and os.path.getsize(path) > 0


def _fresh(path, target, options):
    return not options.forceFlag and not utils.target_needs_rebuild([path], target)


def vcf_inputs(sample_dir, options):
    """(metric, path) of the four VCF files in the order collect_metrics looks at them."""
    return [("phase1Snps", os.path.join(sample_dir, "var.flt.vcf")),
            ("phase1SnpsPreserved", os.path.join(sample_dir, "var.flt_preserved.vcf")),
            ("snps", os.path.join(sample_dir, options.consensusVcfFileName)),
            ("snpsPreserved", os.path.join(sample_dir, options.consensusPreservedVcfFileName))]


def stale_inputs(sample_dir, options):
    """What a collect_one of this sample would have to read on the device: (pileup path or None, [VCF paths]) — the inputs
    that exist, are not empty and whose value the metrics file does not hold freshly.  The phase-2 file of a flow whose fresh
    phase-1 count exceeds --maxsnps is left out: the sample is excluded and that value stays blank (collect_metrics.py:396, :415).
    (Where the phase-1 count is not known yet, the phase-2 file of a sample that turns out to be excluded is counted for nothing.)"""
    target = metrics_path(sample_dir, options)
    try:
        metrics = read_properties(target)
    except IOError:
        metrics = {}
    pileup = os.path.join(sample_dir, "reads.all.pileup")
    want_pileup = _usable(pileup) and not (_fresh(pileup, target, options) and metrics.get("avePileupDepth", ""))
    inputs = vcf_inputs(sample_dir, options)
    vcfs, excluded = [], [False, False]
    for i, (key, path) in enumerate(inputs):
        held = metrics.get(key, "") if _usable(path) and _fresh(path, target, options) else ""
        if i < 2 and held.isdigit() and options.maxSnps > 0 and int(held) > options.maxSnps:
            excluded[i] = True
        if _usable(path) and not held and not (i >= 2 and excluded[i - 2]):
            vcfs.append(path)
    return (pileup if want_pileup else None), vcfs


def collect_one(sample_dir, reference, options, known=None):
    """The metrics file of one sample: the values of collect_metrics.py:467-487 in that order and spelling, written to
    options.metricsFile inside the sample directory and returned as a list of (name, text).  `known`: values a caller has
    just computed, taken instead of reading the input again — "depth_sum" (int), "reference_length" (int), "missingPos",
    "missingPosPreserved" (int), "snp_counts" {VCF path: int}, "count_snps" (callable: [paths] -> [counts], for whatever
    "snp_counts" lacks).  A value the metrics file holds freshly is reused first, as in the reference."""
    known = known or {}
    errors = []

    def handle_error(message):
        verbose_print(message)
        errors.append(message)

    def verify_input_file(prefix, path):                        # collect_metrics.py:51-57
        base = os.path.basename(path)
        if not os.path.isfile(path):
            handle_error(prefix + " " + base + " was not found.")
            return False
        if os.path.getsize(path) == 0:
            handle_error(prefix + " " + base + " is empty.")
            return False
        return True

    target = metrics_path(sample_dir, options)
    sample_id = os.path.basename(os.path.abspath(sample_dir))
    try:
        metrics = read_properties(target)
    except IOError:
        metrics = {}

    def reuse(path, key):
        return metrics.get(key, "") if _fresh(path, target, options) else ""

    machine = flowcell = ""
    fastq_files = [f for f in list_fastq_files(sample_dir) if os.path.isfile(f)]
    if not fastq_files:
        handle_error("No fastq files were found.")
    else:
        tags = extract_metadata_tags(fastq_files[0])
        if tags:
            machine, flowcell = tags[0] or "", tags[1] or ""
    fastq_file_size = sum(os.path.getsize(f) for f in fastq_files) if fastq_files else ""
    fastq_file_list = ", ".join(os.path.basename(f) for f in fastq_files)

    have_samtools = shutil.which("samtools") is not None
    num_reads = percent_mapped = percent_proper = ave_insert = ""
    path = os.path.join(sample_dir, "reads.sam")
    if verify_input_file("SAM file", path):
        if _fresh(path, target, options):
            num_reads, percent_mapped = metrics.get("numberReads", ""), metrics.get("percentReadsMapped", "")
            percent_proper, ave_insert = metrics.get("percentProperPair", ""), metrics.get("aveInsertSize", "")
        if not all([num_reads, percent_mapped, percent_proper, ave_insert]):
            if have_samtools:
                stats = subprocess.run(["samtools", "stats", path], stdout=subprocess.PIPE, universal_newlines=True).stdout
                for line in stats.split("\n"):
                    lower, cells = line.lower(), line.strip().split("\t")
                    if "raw total sequences:" in lower:
                        num_reads = cells[2]
                    elif "reads mapped:" in lower or "reads properly paired:" in lower:
                        try:
                            text = "%.2f" % (100.0 * float(cells[2]) / float(num_reads))
                        except ValueError:
                            text = ""
                        if "reads mapped:" in lower:
                            percent_mapped = text
                        else:
                            percent_proper = text
                    elif "insert size average:" in lower:
                        ave_insert = cells[2]
            missing = [text for value, text in ((num_reads, "number of reads"), (percent_mapped, "percent reads mapped"),
                                                (percent_proper, "percent proper pair"), (ave_insert, "ave insert size")) if not value]
            if missing:
                handle_error("Cannot calculate " + ", ".join(missing) + ".")

    num_dup_reads = ""
    if (os.environ.get("RemoveDuplicateReads") or "true").lower() == "true":
        path = os.path.join(sample_dir, "reads.sorted.deduped.bam")
        if verify_input_file("Deduped BAM file", path):
            num_dup_reads = reuse(path, "numberDupReads")
            if not num_dup_reads and have_samtools:
                num_dup_reads = subprocess.run(["samtools", "view", "-S", "-c", "-f", "1024", path], stdout=subprocess.PIPE,
                                               universal_newlines=True).stdout.strip()

    ave_pileup_depth = ""
    path = os.path.join(sample_dir, "reads.all.pileup")
    if verify_input_file("Pileup file", path):
        ave_pileup_depth = reuse(path, "avePileupDepth")
        if not ave_pileup_depth:
            depth_sum = known["depth_sum"] if "depth_sum" in known else pileup_depth_sum_python(path)
            reference_length = known["reference_length"] if "reference_length" in known else sum(utils.read_fasta_lengths(reference).values())
            if depth_sum > 0 and reference_length > 0:
                ave_pileup_depth = "%.2f" % (float(depth_sum) / float(reference_length))
            else:
                handle_error("Cannot calculate mean pileup depth.")

    def snp_count(path):
        counts = known.get("snp_counts") or {}
        if path in counts:
            return counts[path]
        if "count_snps" not in known:
            raise RuntimeError("no SNP count for %s: collect_one counts on the device (known['count_snps'])" % path)
        res = known["count_snps"]([path])[0]
        if isinstance(res, Exception):
            raise res
        return res

    inputs = vcf_inputs(sample_dir, options)
    values = {}
    excluded = {}
    for (key, path), excl_key, text in ((inputs[0], "excludedSample", "Excluded: exceeded %i maxsnps."),
                                        (inputs[1], "excludedSamplePreserved", "Excluded: preserved exceeded %i maxsnps.")):
        values[key] = excluded[excl_key] = ""
        if verify_input_file("VCF file", path):
            count = reuse(path, key) or snp_count(path)
            # (the reference compares a reused value, a string, with the number and stops with a TypeError: the number is meant)
            if options.maxSnps > 0 and int(count) > options.maxSnps:
                excluded[excl_key] = "Excluded"
                handle_error(text % options.maxSnps)
            values[key] = str(count)
    for (key, path), excl_key in ((inputs[2], "excludedSample"), (inputs[3], "excludedSamplePreserved")):
        values[key] = ""
        if verify_input_file("Consensus VCF file", path) and excluded[excl_key] != "Excluded":
            values[key] = reuse(path, key) or str(snp_count(path))
    for key, name, excl_key in (("missingPos", options.consensusFastaFileName, "excludedSample"),
                                ("missingPosPreserved", options.consensusPreservedFastaFileName, "excludedSamplePreserved")):
        values[key] = ""
        path = os.path.join(sample_dir, name)
        if verify_input_file("Consensus fasta file", path) and excluded[excl_key] != "Excluded":
            values[key] = reuse(path, key) or str(known[key] if key in known else count_missing_positions(path, sample_id))

    rows = [("sample", '"' + sample_id + '"'), ("fastqFileList", '"' + fastq_file_list + '"'), ("fastqFileSize", str(fastq_file_size)),
            ("machine", machine), ("flowcell", flowcell), ("numberReads", num_reads), ("numberDupReads", num_dup_reads),
            ("percentReadsMapped", percent_mapped), ("percentProperPair", percent_proper), ("aveInsertSize", ave_insert),
            ("avePileupDepth", ave_pileup_depth), ("phase1Snps", values["phase1Snps"]), ("phase1SnpsPreserved", values["phase1SnpsPreserved"]),
            ("snps", values["snps"]), ("snpsPreserved", values["snpsPreserved"]), ("missingPos", values["missingPos"]),
            ("missingPosPreserved", values["missingPosPreserved"]), ("excludedSample", excluded["excludedSample"]),
            ("excludedSamplePreserved", excluded["excludedSamplePreserved"]), ("errorList", '"' + " ".join(errors) + '"')]
    with open(target, "w") as f:
        for name, text in rows:
            f.write(name + "=" + text + "\n")
    return rows


# ---- the table -----------------------------------------------------------------------------------------------------------------
def combine(sample_dirs, name, out_path, space_headings=False):
    """metrics.tsv (combine_metrics.py:67-113): a heading row, then one row per sample directory from its metrics file `name`;
    a missing or empty metrics file gives a one-line message in the table and a sample warning."""
    with open(out_path, "w") as f:
        headings = COLUMN_HEADINGS if space_headings else [h.replace(" ", "_") for h in COLUMN_HEADINGS]
        f.write("\t".join(headings) + "\n")
        for d in sample_dirs:
            path = os.path.join(d, name)
            verbose_print("Processing " + path)
            message = None
            if not os.path.isfile(path):
                message = "Sample metrics file %s does not exist." % path
            elif os.path.getsize(path) == 0:
                message = "Sample metrics file %s is empty." % path
            if message:
                f.write(message + "\n")
                sample_warning(message)
                continue
            metrics = read_properties(path)
            cells = []
            for key in METRIC_NAMES:
                text = metrics.get(key, "")
                cells.append('"' + text + '"' if key in QUOTED_METRICS and text else text)
            f.write("\t".join(cells) + "\n")


def sample_warning(message):
    """utils.sample_warning of the reference (utils.py:519-539): into the error log, never a reason to stop."""
    utils._append_error_log(["%s warning:" % utils.program_name_with_command(), message, "=" * 80])
    sys.stdout.flush()
    if message:
        print(message, file=sys.stderr)


# ---- the job -------------------------------------------------------------------------------------------------------------------
def _devices():
    from . import device as devmod
    pinned = os.environ.get("SNPGPU_DEVICE", os.environ.get("LOCAL_RANK"))
    return [int(pinned)] if pinned is not None else list(range(max(1, devmod.device_count())))


def device_work(dev, pileups, vcfs):
    """ONE stream of pileups (depth sums) and ONE stream of VCF files (SNP counts) on a device.  Returns ({pileup: depth sum},
    {vcf: count or IOError}, [pileups the scan refused, summed by the Python loop instead])."""
    from . import device as devmod
    from . import _lib as L
    depth, fallbacks = {}, []
    if pileups:
        ss = dev.siteset([(b"-", 0)], [L.SITE_IN_SNPLIST])     # the scan wants a site set; the depth column needs none
        try:
            results, rcs, _ = dev.call_consensus_files(ss, pileups, devmod.make_params(), want_depth_sum=True)
        finally:
            ss.close()
        for path, res, rc in zip(pileups, results, rcs):        # a pileup the scan refuses: the reference's own loop skips bad lines
            if rc == 0:
                depth[path] = res.depth_sum
            else:
                verbose_print("# the pileup scan refused %s (%d): its depth column is summed on the host" % (path, rc))
                depth[path] = pileup_depth_sum_python(path)
                fallbacks.append(path)
    counts = dict(zip(vcfs, count_snps_files(dev, vcfs))) if vcfs else {}
    return depth, counts, fallbacks


def run_batch(sample_dirs, reference, options, merged_path=None, space_headings=False, devices=None, known=None, report_errors=True):
    """Every sample's metrics file, then (merged_path) the table.  devices: open Device objects to use (default: one per
    visible GPU, opened only when something has to be read there, closed afterwards); known: {sample dir: dict} as
    collect_one takes them; report_errors=False: sample errors are only returned.  Returns {"failed", "pileups_summed",
    "vcf_files_counted", "depth_fallbacks" (pileups the scan refused), "errors" {sample dir: message}}."""
    import concurrent.futures
    import threading
    from . import device as devmod
    known = known or {}
    good = []
    failed = 0
    sample_errors, fallbacks = {}, []

    def sample_error(d, message):
        sample_errors[d] = message
        if report_errors:
            utils.sample_error(message, continue_possible=True)
    for d in sample_dirs:                                       # collect_metrics.py:180
        message = None
        if not os.path.exists(d):
            message = "Sample directory " + d + " does not exist."
        elif not os.path.isdir(d):
            message = "Sample directory " + d + " is not a directory."
        elif not os.listdir(d):
            message = "Sample directory " + d + " is empty."
        if message:
            sample_error(d, message)
            failed += 1
        else:
            good.append(d)

    pileups, vcfs = [], []
    for d in good:
        k = known.get(d) or {}
        pileup, stale = stale_inputs(d, options)
        if pileup and "depth_sum" not in k:
            pileups.append(pileup)
        vcfs.extend(p for p in stale if p not in (k.get("snp_counts") or {}))
    depth, counts = {}, {}
    if pileups or vcfs:
        own = devices is None
        devs = devices if not own else [devmod.Device(i) for i in _devices()[:max(len(pileups), len(vcfs))]]
        lock, errors = threading.Lock(), []

        def worker(dev, my_pileups, my_vcfs):
            try:
                dp, ct, fb = device_work(dev, my_pileups, my_vcfs)
                with lock:
                    depth.update(dp)
                    counts.update(ct)
                    fallbacks.extend(fb)
            except Exception as err:                            # noqa: B902 — reported below, in the main thread
                with lock:
                    errors.append(err)
        try:
            threads = [threading.Thread(target=worker, args=(dv, pileups[i::len(devs)], vcfs[i::len(devs)])) for i, dv in enumerate(devs)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        finally:
            if own:
                for dv in devs:
                    dv.close()
        if errors:
            raise errors[0]
    reference_length = sum(utils.read_fasta_lengths(reference).values()) if good else 0

    def one(d):
        k = dict(known.get(d) or {})
        k.setdefault("reference_length", reference_length)
        pileup = os.path.join(d, "reads.all.pileup")
        if pileup in depth:
            k["depth_sum"] = depth[pileup]
        mine = dict(k.get("snp_counts") or {})
        for _, path in vcf_inputs(d, options):
            if path in counts and path not in mine:
                if isinstance(counts[path], Exception):
                    raise counts[path]
                mine[path] = counts[path]
        k["snp_counts"] = mine
        collect_one(d, reference, options, k)

    with concurrent.futures.ThreadPoolExecutor(max_workers=devmod.host_threads(16)) as ex:
        futures = [(d, ex.submit(one, d)) for d in good]
        for d, fut in futures:
            err = fut.exception()
            if err is not None:
                sample_error(d, "Error: collect_metrics failed for sample %s: %s: %s" % (os.path.basename(os.path.abspath(d)), type(err).__name__, err))
                failed += 1
    if merged_path:
        combine(sample_dirs, options.metricsFile, merged_path, space_headings)
    return {"failed": failed, "pileups_summed": len(pileups), "vcf_files_counted": len(vcfs), "depth_fallbacks": len(fallbacks), "errors": sample_errors}


def add_arguments(sub):
    sub.add_argument(dest="sampleDirsFile", type=str, help="Relative or absolute path to file containing a list of directories -- one per sample")
    sub.add_argument(dest="referenceFile", type=str, help="Relative or absolute path to the reference fasta file")
    sub.add_argument("-f", "--force", dest="forceFlag", action="store_true", help="Force processing even when result files already exist and are newer than inputs")
    sub.add_argument("-o", "--output", dest="metricsFile", type=str, default="metrics", metavar="NAME", help="Output file name of the metrics file in each sample directory")
    sub.add_argument("-m", "--maxsnps", dest="maxSnps", type=int, default=-1, metavar="INT", help="Maximum allowed number of SNPs per sample")
    sub.add_argument("-c", dest="consensusFastaFileName", type=str, default="consensus.fasta", metavar="NAME", help="File name of the consensus fasta file which must exist in the sample directory")
    sub.add_argument("-C", dest="consensusPreservedFastaFileName", type=str, default="consensus_preserved.fasta", metavar="NAME", help="File name of the consensus preserved fasta file which must exist in the sample directory")
    sub.add_argument("-v", dest="consensusVcfFileName", type=str, default="consensus.vcf", metavar="NAME", help="File name of the consensus vcf file which must exist in the sample directory")
    sub.add_argument("-V", dest="consensusPreservedVcfFileName", type=str, default="consensus_preserved.vcf", metavar="NAME", help="File name of the consensus preserved vcf file which must exist in the sample directory")
    sub.add_argument("--verbose", dest="verbose", type=int, default=1, metavar="0..5", help="Verbose message level (0=no info, 5=lots)")
    sub.add_argument("--mergedMetricsFile", dest="mergedMetricsFile", type=str, default=None, metavar="PATH", help="Also write the table of all samples' metrics (combine_metrics) to this file")
    sub.add_argument("-s", "--spaces", dest="spaceHeadings", action="store_true", help="Emit column headings with spaces instead of underscores")


def collect_metrics_batch(args):
    """Entry point of ``cfsan_snp_pipeline collect_metrics_batch``."""
    utils.print_log_header(classpath=True)
    utils.print_arguments(args)
    utils.verify_non_empty_input_files("Reference file", [args.referenceFile], error_handler="global")
    if utils.verify_non_empty_input_files("File of sample directories", [args.sampleDirsFile]) > 0:
        utils.global_error(None)
    with open(args.sampleDirsFile, "r") as f:
        sample_dirs = [d for d in (line.rstrip() for line in f) if d]
    done = run_batch(sample_dirs, args.referenceFile, Options.from_args(args), args.mergedMetricsFile, args.spaceHeadings)
    verbose_print("# %d pileups summed, %d VCF files counted on the device" % (done["pileups_summed"], done["vcf_files_counted"]))
    if done["failed"]:
        verbose_print("%d of %d samples failed." % (done["failed"], len(sample_dirs)))
