"""``cfsan_snp_pipeline merge_vcfs`` — the multi-sample snpma.vcf from the per-sample consensus.vcf files.

The reference copies every file, runs bgzip and tabix on each copy and then ``bcftools merge --merge all --info-rules NS:sum``
over all of them (merge_vcfs.py:96-139).  Here the step has two routes (--vcfMerger / SNPGPU_VCF_MERGER):

  bcftools   the reference's own commands, character for character
  device     the library's merge (csrc/vcf_merge.hip): parse, merge and format on the GPU, file to file
  auto       bcftools when bgzip, tabix and bcftools are all on PATH, else device

What the device route computes is pinned on the pipeline's OWN VCF grammar only — one sample column, haploid GT, FORMAT
GT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT, INFO NS=<n>, ID and QUAL '.', alleles of one byte — by the four snpma files the reference
ships.  Outside that grammar nothing pins the rule, and a line outside it ends the run with an error that names it.

  parse_line / merge_row / merge_texts   the merge as plain text processing, one row at a time: the statement the kernels are
                                         held against
  merge_files_device                     the library call + header
  merge_vcfs                             the subcommand (merge_vcfs.py:44-99 of the reference)
"""
from __future__ import print_function

import argparse
import os
import re
import resource
import shutil
import subprocess
import sys
import tempfile

from . import utils
from .utils import verbose_print

FORMAT_IDS = b"GT:SDP:RD:AD:RDF:RDR:ADF:ADR:FT"
ABSENT_CELL = b".:.:.:.:.:.:.:.:."
MAX_ALT = 8                         # ALT symbols of one record: what a record of the writer holds (SNPGPU_MAX_SYMS)
MAX_FILTERS = 31                    # ##FILTER ids besides PASS
DEFAULT_PARAMS = "--merge all --info-rules NS:sum"
MERGERS = ("bcftools", "device", "auto")
TOOLS = ("bgzip", "tabix", "bcftools")
DOT = 0xFFFFFFFF                    # a '.' inside a Number=A vector
_COUNT = re.compile(br"[0-9]{1,10}\Z")
_FILTER_ID = re.compile(br"##FILTER=<ID=([^,>]+)")


class MergeError(ValueError):
    """A line, or a site, outside the grammar the merge rule is pinned on."""


class Cell(object):
    __slots__ = ("chrom", "pos", "ref", "alts", "filters", "ns", "gt", "sdp", "rd", "rdf", "rdr", "ad", "adf", "adr")


def _count(text, what):
    if not _COUNT.match(text) or int(text) >= DOT:
        raise MergeError("%s is not a count below 2^32 - 1" % what)
    return int(text)


def parse_line(line, filter_ids):
    """The record of one data line (bytes, no terminator) of the writer's grammar; MergeError when it is outside it.
    filter_ids: the ##FILTER ids of the header besides PASS, in header order."""
    cols = line.split(b"\t")
    if len(cols) != 10:
        raise MergeError("not ten TAB-separated columns (one sample column)")
    chrom, pos, vid, ref, alt, qual, flt, info, fmt, sample = cols
    c = Cell()
    if not chrom:
        raise MergeError("empty CHROM")
    c.chrom = chrom
    c.pos = _count(pos, "POS")
    if vid != b"." or qual != b".":
        raise MergeError("ID and QUAL are not '.'")
    if len(ref) != 1 or ref in b".,":
        raise MergeError("REF is not one byte")
    c.ref = ref
    c.alts = [] if alt == b"." else alt.split(b",")
    if len(c.alts) > MAX_ALT or any(len(a) != 1 or a == b"." or a == ref for a in c.alts) or len(set(c.alts)) != len(c.alts):
        raise MergeError("ALT is not '.' or up to %d distinct one-byte alleles other than REF" % MAX_ALT)
    if not info.startswith(b"NS="):
        raise MergeError("INFO is not NS=<n>")
    c.ns = _count(info[3:], "NS")
    if fmt != FORMAT_IDS:
        raise MergeError("FORMAT is not %s" % FORMAT_IDS.decode())
    vals = sample.split(b":")
    if len(vals) != 9:
        raise MergeError("the sample column has not nine fields")
    gt, sdp, rd, ad, rdf, rdr, adf, adr, ft = vals
    if gt == b".":
        c.gt = None
    else:
        if len(gt) != 1 or not gt.isdigit() or int(gt) > len(c.alts):
            raise MergeError("GT is not '.' or the index of one allele")
        c.gt = int(gt)
    c.sdp, c.rd, c.rdf, c.rdr = _count(sdp, "SDP"), _count(rd, "RD"), _count(rdf, "RDF"), _count(rdr, "RDR")
    vectors = []
    for name, text in ((b"AD", ad), (b"ADF", adf), (b"ADR", adr)):
        items = text.split(b",")
        if len(items) != max(1, len(c.alts)):
            raise MergeError("%s has not one value per ALT allele" % name.decode())
        values = [DOT if v == b"." else _count(v, name.decode()) for v in items]      # (under ALT '.' the one value is held to the rule and dropped)
        vectors.append(values if c.alts else [])
    c.ad, c.adf, c.adr = vectors
    if ft != flt:
        raise MergeError("FILTER and FT differ")
    if ft == b"PASS":
        c.filters = []
    else:
        try:
            c.filters = [filter_ids.index(f) for f in ft.split(b";")]
        except ValueError:
            raise MergeError("FT names a filter the header of the first file does not define")
        if any(a >= b for a, b in zip(c.filters, c.filters[1:])):
            raise MergeError("the filters of FT are not in header order")
    return c


def merge_row(cells, filter_ids):
    """One merged row (bytes, no terminator) from the records of one (CHROM, POS): cells[column] is a Cell or None."""
    present = [c for c in cells if c is not None]
    first = present[0]
    if any(c.ref != first.ref for c in present):
        raise MergeError("records of different REF at %s:%d" % (first.chrom.decode("latin-1"), first.pos))
    alts, filters, ns = [], [], 0
    for c in present:                                         # unions in order of first appearance over the columns
        alts.extend(a for a in c.alts if a not in alts)
        filters.extend(f for f in c.filters if f not in filters)
        ns += c.ns
    flt = b";".join(filter_ids[f] for f in filters) if filters else b"PASS"      # (PASS leaves a union that holds anything else)
    out = [first.chrom, b"%d" % first.pos, b".", first.ref, b",".join(alts) if alts else b".", b".", flt, b"NS=%d" % ns, FORMAT_IDS]
    for c in cells:
        if c is None:
            out.append(ABSENT_CELL)
            continue
        gt = b"." if c.gt is None else (b"0" if c.gt == 0 else b"%d" % (1 + alts.index(c.alts[c.gt - 1])))

        def vector(own):
            if not alts:
                return b"."
            at = {a: v for a, v in zip(c.alts, own)}
            return b",".join(b"." if at.get(a, DOT) == DOT else b"%d" % at[a] for a in alts)
        ft = b";".join(filter_ids[f] for f in c.filters) if c.filters else b"PASS"
        out.append(b":".join([gt, b"%d" % c.sdp, b"%d" % c.rd, vector(c.ad), b"%d" % c.rdf, b"%d" % c.rdr, vector(c.adf), vector(c.adr), ft]))
    return b"\t".join(out)


def split_vcf(data):
    """(header lines without terminators up to and without #CHROM, the #CHROM line, [(offset, data line)]) of VCF text."""
    header, chrom_line, rows = [], None, []
    at, n = 0, len(data)
    while at < n:
        end = data.find(b"\n", at)
        if end < 0:
            end = n
        line = data[at:end - 1] if end > at and data[end - 1:end] == b"\r" else data[at:end]
        if line.startswith(b"#"):
            if chrom_line is None:
                if line.startswith(b"#CHROM"):
                    chrom_line = line
                else:
                    header.append(line)
        elif line:
            rows.append((at, line))
        at = end + 1
    return header, chrom_line, rows


def filter_ids_of(header):
    return [m.group(1) for m in (_FILTER_ID.match(h) for h in header) if m and m.group(1) != b"PASS"]


def sample_name_of(chrom_line, where):
    cols = (chrom_line or b"").split(b"\t")
    if len(cols) != 10:
        raise MergeError("%s: no #CHROM line with one sample column" % where)
    return cols[9]


def merged_header(first_header, contigs, names, own_lines):
    """The header of the merged file: the first file's header with the PASS filter on line 2, a contig line per contig, the lines
    of the merger itself, then #CHROM with every column."""
    pass_line = b'##FILTER=<ID=PASS,Description="All filters passed">'
    lines = [h for h in first_header if h != pass_line]
    lines.insert(1 if lines and lines[0].startswith(b"##fileformat") else 0, pass_line)
    lines.extend(b"##contig=<ID=" + c + b">" for c in contigs)
    lines.extend(own_lines)
    lines.append(b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] + list(names)))
    return b"\n".join(lines) + b"\n"


def own_header_lines(command=""):
    return [b"##snpgpu_mergeVersion=" + utils.__version__.encode(), b"##snpgpu_mergeCommand=" + command.encode("utf-8", "surrogateescape")]


def merge_texts(texts, own_lines=(), names_of_files=None):
    """The whole merge on the host: texts[column] is the VCF text (bytes) of one sample, in column order."""
    parts = [split_vcf(t) for t in texts]
    where = names_of_files or ["file %d" % i for i in range(len(texts))]
    filter_ids = filter_ids_of(parts[0][0])
    if len(filter_ids) > MAX_FILTERS:
        raise MergeError("%s: more than %d filters" % (where[0], MAX_FILTERS))
    names = [sample_name_of(p[1], w) for p, w in zip(parts, where)]
    contigs, sites = [], {}
    for col, (p, w) in enumerate(zip(parts, where)):
        for off, line in p[2]:
            try:
                c = parse_line(line, filter_ids)
            except MergeError as err:
                raise MergeError("%s: the line at byte %d is outside the pipeline's own VCF grammar: %s" % (w, off, err))
            if c.chrom not in contigs:
                contigs.append(c.chrom)
            row = sites.setdefault((contigs.index(c.chrom), c.pos), [None] * len(texts))
            if row[col] is not None:
                raise MergeError("%s: the position %s:%d comes twice" % (w, c.chrom.decode("latin-1"), c.pos))
            row[col] = c
    out = [merged_header(parts[0][0], contigs, names, list(own_lines))]
    for key in sorted(sites):
        out.append(merge_row(sites[key], filter_ids) + b"\n")
    return b"".join(out)


def merge_files_python(paths, out_path, own_lines=()):
    texts = []
    for p in paths:
        with open(p, "rb") as f:
            texts.append(f.read())
    data = merge_texts(texts, own_lines, list(paths))
    with open(out_path, "wb") as f:
        f.write(data)


def column_order(sample_dirs):
    """The order of the merged columns: the shell's expansion of <tmp>/*.gz, that is sorted by basename(sampleDir) + '.vcf.gz'
    (bytewise: the C locale), not the order of sampleDirsFile.  Directories of one basename stand for one copy: the last wins."""
    by_name = {}
    for d in sample_dirs:
        by_name[os.path.basename(d) + ".vcf.gz"] = d
    return [by_name[k] for k in sorted(by_name, key=lambda s: s.encode("utf-8", "surrogateescape"))]


def merge_files_device(dev, paths, out_path, command="", device_bytes=0):
    """The library's merge of `paths` (column order) into out_path.  Returns its statistics (device.MergeStats as a dict).
    device_bytes: the budget of --mergeDeviceBytes, handed on only when it is set."""
    own = b"\n".join(own_header_lines(command)) + b"\n"
    if device_bytes:
        return dev.merge_vcf_files(paths, out_path, own, device_bytes=device_bytes)
    return dev.merge_vcf_files(paths, out_path, own)


# ---- the routes --------------------------------------------------------------------------------------------------------------
def have_tools():
    return all(shutil.which(t) for t in TOOLS)


def choose_merger(asked=None):
    mode = asked or os.environ.get("SNPGPU_VCF_MERGER") or "auto"
    if mode not in MERGERS:
        utils.global_error("Error: --vcfMerger / SNPGPU_VCF_MERGER must be one of %s, not %s." % (", ".join(MERGERS), mode))
    if mode == "auto":
        mode = "bcftools" if have_tools() else "device"
    return mode


def merge_device_bytes(asked=None):
    """--mergeDeviceBytes / SNPGPU_MERGE_DEVICE_BYTES: the device memory the device route may allocate (0: what is free, less a
    reserve).  Where the records of all files do not fit it the merge runs in bounded memory, a key pass and rounds of sites."""
    value = asked if asked is not None else (os.environ.get("SNPGPU_MERGE_DEVICE_BYTES") or "0")
    text = str(value).strip()
    if not (text.isascii() and text.isdigit()):
        utils.global_error("Error: --mergeDeviceBytes / SNPGPU_MERGE_DEVICE_BYTES must be a non-negative integer, not %s." % value)
    return int(text)


def _run(command_line, stdout):
    """command.run of the reference: the line goes through the shell (shell=True), which expands <tmp>/*.gz in its own
    collating order and honours whatever shell syntax BcftoolsMerge_ExtraParams holds."""
    sys.stdout.flush()
    subprocess.check_call(command_line, stdout=stdout, shell=True)


def merge_bcftools(sample_dirs, good, vcf_name, merged):
    """merge_vcfs.py:101-139 of the reference."""
    for tool in TOOLS:
        if not shutil.which(tool):
            utils.global_error("Error: %s is not on the path" % tool)
    verbose_print("# %s Copying VCF files to temp directory" % utils.timestamp())
    temp_dir = tempfile.mkdtemp(prefix="tmp.vcf.", dir=os.path.dirname(merged))
    copies = []
    for d in sample_dirs:
        src = os.path.join(d, vcf_name)
        if src in good:
            dst = os.path.join(temp_dir, os.path.basename(d) + ".vcf")
            copies.append(dst)
            verbose_print("copy %s %s" % (src, dst))
            shutil.copy2(src, dst)
    verbose_print("# %s Compressing VCF files" % utils.timestamp())
    for path in copies:
        verbose_print("bgzip -c %s > %s" % (path, path + ".gz"))
        with open(path + ".gz", "wb") as f:
            _run("bgzip -c " + path, f)
    verbose_print("# %s Indexing VCF files" % utils.timestamp())
    for path in copies:
        verbose_print("tabix -f -p vcf " + path + ".gz")
        _run("tabix -f -p vcf " + path + ".gz", sys.stdout)
    params = os.environ.get("BcftoolsMerge_ExtraParams") or DEFAULT_PARAMS
    verbose_print("# %s Merging VCF files" % utils.timestamp())
    command_line = "bcftools merge -o " + merged + " " + params + " " + temp_dir + "/*.gz"
    verbose_print(command_line)
    _run(command_line, sys.stdout)
    shutil.rmtree(temp_dir)                                   # (as the reference: a failed command leaves the directory to be looked at)


def check_device_params():
    params = os.environ.get("BcftoolsMerge_ExtraParams")
    if params and params.split() != DEFAULT_PARAMS.split():
        utils.global_error("Error: BcftoolsMerge_ExtraParams=%r cannot be honoured by the device route of merge_vcfs, which merges as "
                           "'%s' does; use --vcfMerger bcftools for other parameters." % (params, DEFAULT_PARAMS))


def merge_sample_dirs(sample_dirs, vcf_name, merged, force=False, merger=None, dev=None, device_bytes=None):
    """The step for a list of sample directories (merge_vcfs.py:60-139).  Returns the route that ran: 'fresh', 'copy',
    'bcftools' or 'device'.  device_bytes: --mergeDeviceBytes as given (None: the environment's, else 0)."""
    budget = merge_device_bytes(device_bytes)
    vcf_files = [os.path.join(d, vcf_name) for d in sample_dirs]
    good = []
    for path in vcf_files:
        if not utils.verify_non_empty_input_files("Sample vcf file", [path], error_handler="sample", continue_possible=True):
            good.append(path)
    if not good:
        utils.global_error("There are no vcf files to merge.")
    if not force and not utils.target_needs_rebuild(vcf_files, merged):
        verbose_print("# Multi-VCF file is already freshly created.  Use the -f option to force a rebuild.")
        return "fresh"
    mode = choose_merger(merger)
    if mode == "bcftools":                                    # (the reference raises the limit before it looks at the number of files)
        needed = len(good) + 4
        soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
        if needed > hard:
            utils.global_error("Error: unable to merge the VCF files. %i open files handles are needed, but the hard limit is only %i." % (needed, hard))
        if needed > soft:
            verbose_print("# %s Increasing number of open file descriptors from %i to %i" % (utils.timestamp(), soft, needed))
            resource.setrlimit(resource.RLIMIT_NOFILE, (needed, hard))
    if len(good) == 1:
        shutil.copy(good[0], merged)
        return "copy"
    if mode == "bcftools":
        verbose_print("# merge_vcfs route: bcftools (the reference's commands)")
        if budget:
            verbose_print("# --mergeDeviceBytes %d is ignored: it bounds the device route only" % budget)
        merge_bcftools(sample_dirs, good, vcf_name, merged)
        return "bcftools"
    check_device_params()
    verbose_print("# merge_vcfs route: device (parity pinned on the pipeline's own VCF grammar only)")
    paths = [os.path.join(d, vcf_name) for d in column_order([d for d in sample_dirs if os.path.join(d, vcf_name) in good])]
    own = dev is None
    if own:
        from . import device as devmod
        dev = devmod.Device(int(os.environ.get("SNPGPU_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    try:
        stats = merge_files_device(dev, paths, merged, "merge -o %s %s %s" % (merged, DEFAULT_PARAMS, " ".join(paths)), budget)
    except Exception as err:                                  # noqa: B902 — a line outside the grammar, an unreadable file
        if os.path.exists(merged):
            os.unlink(merged)
        utils.global_error("Error: merge_vcfs failed: %s" % err)
    finally:
        if own:
            dev.close()
    verbose_print("# %d columns, %d sites, %d records (%d of them parsed on the host), %d bytes in %d rounds; parse %.3f s, merge %.3f s, write %.3f s" %
                  (stats["columns"], stats["sites"], stats["cells"], stats["host_lines"], stats["bytes"], stats["rounds"],
                   stats["seconds_parse"], stats["seconds_merge"], stats["seconds_write"]))
    if stats.get("input_passes", 1) > 1:
        verbose_print("# device route, %d site rounds of %d sites, %d readings of the input" % (stats["site_rounds"], stats["sites_per_round"], stats["input_passes"]))
    else:
        verbose_print("# device route, single pass, 1 reading of the input")
    merge_sample_dirs.last_stats = stats
    return "device"


merge_sample_dirs.last_stats = None                           # the library's statistics of the last device merge of this process


def add_arguments(sub):
    sub.add_argument(dest="sampleDirsFile", type=str, help="Relative or absolute path to file containing a list of directories -- one per sample")
    sub.add_argument("-f", "--force", dest="forceFlag", action="store_true", help="Force processing even when result files already exist and are newer than inputs")
    sub.add_argument("-n", "--vcfname", dest="vcfFileName", type=str, default="consensus.vcf", metavar="NAME", help="File name of the vcf files which must exist in each of the sample directories")
    sub.add_argument("-o", "--output", dest="mergedVcfFile", type=str, default="snpma.vcf", metavar="FILE", help="Output file.  Relative or absolute path to the merged multi-vcf file")
    sub.add_argument("--vcfMerger", dest="vcfMerger", type=str, default=None, choices=MERGERS, metavar="MODE",
                     help="Who merges: bcftools (bgzip, tabix and bcftools on PATH, as the reference), device (this build's merge; parity pinned on the pipeline's own VCF grammar only), "
                          "auto (bcftools when all three tools are on PATH, else device).  Default: $SNPGPU_VCF_MERGER, else auto")
    sub.add_argument("--mergeDeviceBytes", dest="mergeDeviceBytes", type=str, default=argparse.SUPPRESS, metavar="INT",
                     help="Device memory the device route may allocate (0 = what is free, less a reserve); where the records of all files do not fit it the merge runs in "
                          "bounded memory: a key pass over the files, then one reading per range of sites.  Ignored by the bcftools route.  Default: $SNPGPU_MERGE_DEVICE_BYTES, else 0")


def merge_vcfs(args):
    """Entry point of ``cfsan_snp_pipeline merge_vcfs``."""
    utils.print_log_header()
    utils.print_arguments(args)
    utils.verify_non_empty_input_files("File of sample directories", [args.sampleDirsFile], error_handler="global")
    with open(args.sampleDirsFile, "r") as f:
        sample_dirs = [d for d in (line.rstrip() for line in f) if d]
    merge_sample_dirs(sample_dirs, args.vcfFileName, args.mergedVcfFile, args.forceFlag, getattr(args, "vcfMerger", None),
                      device_bytes=getattr(args, "mergeDeviceBytes", None))
