"""The drop-in end to end on the GPU box: the reference's OWN dbgh5 (main(), Configuration, Repartitor, processor chain, HDF5 storage), patched with
integration/gatb-core.device.patch + integration/gatb_device/*.hpp and linked against libgkc_hip.so
(integration/check_integration.sh --link -> oracle/_ref/dbgh5_device, a build-container artefact that travels with the repository snapshot), must write
.h5 files whose datasets are exactly what the UNPATCHED reference wrote for the same input (tests/golden/reference_run/*.npz): every /dsk/solid/<p> in order,
the histogram, the repartition table. Three ways through the binding:
  * bulk        the default chain: solidity window + histogram on the device, one block insert per partition (BagHDF5Patch::insert(const Item*, size_t));
  * per record  GATB_DEVICE_NO_BULK=1: every record through the chain's virtual process();
  * iterated    GATB_DEVICE_NO_TEXT=1: the bank is iterated sequence by sequence and packed by the worker threads (what happens for a gzipped or non-FASTA bank);
                by default the text of a plain FASTA / FASTQ bank goes to the device as it is and is parsed there (gkc_push_fastx);
  * two ranks   two processes on the one GPU (the library's file-mailbox transport), reads shared out by index, super-k-mers exchanged, results gathered on
                rank 0: ONE .h5 with every dataset of the single-process file (CountProcessorDump.hpp:85-95, GraphUnitigs.cpp:921-931).
The files are read back with the reference's own gatb-h5dump (oracle/_ref/ref, built by integration/build_reference.sh). Where the artefacts are absent: FAILED on a GPU box (the build step that makes them did not run), skipped elsewhere."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.test_reference_run import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "dbgh5_device")
H5DUMP = os.path.join(ROOT, "oracle", "_ref", "ref", "gatb-h5dump")


def _gpu_box():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:      # noqa
        return False


@pytest.fixture
def artefacts_missing(request):
    pytest.fail("%s: built in the build container by __graft_entry__.build() (integration/build_reference.sh + check_integration.sh --link) and shipped with the "
                "snapshot; on a GPU box their absence is a FAILED build, not a reason to skip a quarter of the suite (VERDICT r5 weak #1)" % request.node.get_closest_marker("missing_artefacts").args[0])


def need(*paths):
    """mark for tests that run a build-container artefact: nothing when it is there; where it is absent the test FAILS on a GPU box and is skipped elsewhere"""
    missing = [os.path.relpath(q, ROOT) for q in paths if not os.path.exists(q)]
    if not missing:
        return lambda f: f
    if _gpu_box():
        return lambda f: pytest.mark.missing_artefacts(", ".join(missing) + " absent")(pytest.mark.usefixtures("artefacts_missing")(f))
    return pytest.mark.skipif(True, reason=", ".join(missing) + " absent (built in the build container: integration/check_integration.sh --link)")


needs_artefacts = need(EXE, H5DUMP)

CASES = {"k21_freq_4parts": (["-minimizer-type", "1", "-repartition-type", "1"], "1", "1"),
         "k21_default_parts": ([], "1", "1"),
         "k31_2parts_mphf": ([], "2000", "2"),
         "k63_neighbor_mphf": ([], "2000", "1"),        # span 64: 32-byte Count records through the bulk insert (DeviceCounting.hpp: sizeof(Count) == recBytes)
         "k31_auto_parts": ([], "1", "1")}              # -abundance-min auto: the cut-off processor + a proxy = TWO processors (SortingCountAlgorithm.cpp:418-444): no bulk plan,
                                                        # every record through process(); the cut-off (Histogram::compute_threshold) and the solid set must be the reference's
ABUNDANCE_MIN = {"k31_auto_parts": "auto"}

# the steps BEHIND the counting step (BASELINE configs[4]: Bloom + MPHF, and what dbgh5 builds on them), flags as the fixture's reference run had them:
#   *_neighbor_mphf  -bloom neighbor -debloom none -branching-nodes none (MPHF on)
#   *_defaults       NO flags at all: MPHF, neighbor Bloom, cascading debloom (DebloomMinimizerAlgorithm: contains8 of every solid k-mer), branching nodes
PIPELINE = {"k31_neighbor_mphf": (["-bloom", "neighbor", "-debloom", "none", "-branching-nodes", "none"], "2000", "1"),
            "k63_neighbor_mphf": (["-bloom", "neighbor", "-debloom", "none", "-branching-nodes", "none"], "2000", "1"),
            "k31_defaults": ([], "2000", "1"),
            "k63_defaults": ([], "2000", "1"),
            "k21_defaults_parts": ([], "1", "1")}


def dump_dataset(h5, path, mode):
    with tempfile.NamedTemporaryFile() as t:
        subprocess.run([H5DUMP, "-d", path, "-b", mode, "-o", t.name, h5], capture_output=True)
        return np.fromfile(t.name, dtype=np.uint8)


def check_h5(h5, tag):
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    rec = 12 if k <= 31 else 20
    assert np.array_equal(dump_dataset(h5, "/minimizers/minimRepart", "LE"), z["minimRepart"]), "minimRepart differs"
    for p in range(nbpart):
        raw = dump_dataset(h5, "/dsk/solid/%d" % p, "FILE")
        n = len(raw) // rec; raw = raw[:n * rec].reshape(n, rec)
        vals = [int.from_bytes(bytes(r), "little") for r in raw[:, :rec - 4]]
        ab = raw[:, rec - 4:].copy().view("<u4")[:, 0].tolist()
        assert list(zip(vals, ab)) == parts[p], "/dsk/solid/%d differs from the unpatched reference's" % p
    hist = dump_dataset(h5, "/histogram/histogram", "FILE"); hist = hist[:len(hist) // 12 * 12].reshape(-1, 12)
    assert np.array_equal(hist[:, 4:].copy().view("<u8")[:, 0], z["histogram_abundance"]), "histogram differs"
    assert int(dump_dataset(h5, "/histogram/cutoff", "LE").view("<u8")[0]) == int(z["cutoff"]), "cut-off differs"
    assert int(dump_dataset(h5, "/histogram/nbsolidsforcutoff", "LE").view("<u8")[0]) == int(z["nbsolidsforcutoff"]), "nbsolidsforcutoff differs"


def fasta_to_fastq(text):
    """the same reads as FASTQ; every third quality line starts with '@' (a record start must not be taken for one: DeviceSession::recordStart)"""
    out, name, seq, n = [], None, [], 0
    def flush():
        nonlocal n
        if name is not None:
            sq = b"".join(seq)
            out.append(b"@" + name + b"\n" + sq + b"\n+\n" + ((b"@" + b"I" * (len(sq) - 1)) if n % 3 == 0 and sq else b"I" * len(sq)) + b"\n"); n += 1
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            flush(); name = line[1:]; seq = []
        elif line:
            seq.append(line.strip())
    flush()
    return b"".join(out)


COUNT_ONLY = ["-bloom", "none", "-debloom", "none", "-branching-nodes", "none", "-no-mphf"]


def run_dbgh5(tag, outdir, env_extra=None, out_name=None, fastq=False, pipeline=False):
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    extra, mem, cores = (PIPELINE if pipeline else CASES)[tag]
    fa = os.path.join(outdir, tag + (".fq" if fastq else ".fa"))
    if not os.path.exists(fa):
        open(fa, "wb").write(fasta_to_fastq(bytes(z["fasta"])) if fastq else bytes(z["fasta"]))
    out = os.path.join(outdir, out_name or (tag + "_dev"))
    cmd = [EXE, "-in", fa, "-kmer-size", str(k), "-abundance-min", ABUNDANCE_MIN.get(tag, "2"), "-out", out, "-out-tmp", outdir, "-nb-cores", cores,
           "-max-memory", mem, "-verbose", "0"] + ([] if pipeline else COUNT_ONLY) + extra
    # GATB_DEVICE_REFERENCE_CONFIG: partitions and passes as the reference derives them from -max-memory / -nb-cores (the fixtures' layout); without it the patched
    # ConfigurationAlgorithm sizes them from the HBM of the device (test_configuration_sized_from_the_device below)
    env = dict(os.environ); env["GATB_DEVICE_REFERENCE_CONFIG"] = "1"; env.update(env_extra or {})
    if env.get("GATB_DEVICE_REFERENCE_CONFIG") == "0":
        del env["GATB_DEVICE_REFERENCE_CONFIG"]
    return subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out + ".h5"


@needs_artefacts
@pytest.mark.parametrize("tag", sorted(CASES))
@pytest.mark.parametrize("mode", ["bulk", "per_record", "iterated", "fastq"])
def test_patched_dbgh5_writes_the_reference_datasets(tmp_path, tag, mode):
    p, h5 = run_dbgh5(tag, str(tmp_path), {"per_record": {"GATB_DEVICE_NO_BULK": "1"}, "iterated": {"GATB_DEVICE_NO_TEXT": "1"}}.get(mode), fastq=mode == "fastq")
    log = p.communicate(timeout=600)[0]
    assert p.returncode == 0, log[-2000:]
    check_h5(h5, tag)


@needs_artefacts
@pytest.mark.parametrize("tag,how", [("k21_freq_4parts", "text"), ("k31_2parts_mphf", "text"), ("k21_default_parts", "fastq"), ("k31_2parts_mphf", "iterated")])
def test_two_ranks_write_one_h5(tmp_path, tag, how):
    """how: text = every rank parses its own byte range of the FASTA file on the device; fastq = the same on a FASTQ version of the reads (record starts found among
    quality lines that begin with '@'); iterated = every rank iterates the bank and keeps the reads whose index is its rank modulo 2"""
    box = tmp_path / "box"; box.mkdir()
    procs = []
    for r in range(2):
        env = {"GATB_DEVICE_RANKS": "2", "GATB_DEVICE_RANK": str(r), "GATB_DEVICE_TRANSPORT_DIR": str(box)}
        if how == "iterated":
            env["GATB_DEVICE_NO_TEXT"] = "1"
        procs.append(run_dbgh5(tag, str(tmp_path), env, out_name="%s_rank%d" % (tag, r), fastq=how == "fastq"))
    logs = [p.communicate(timeout=900)[0] for p, _ in procs]
    assert all(p.returncode == 0 for p, _ in procs), "\n".join(l[-1500:] for l in logs)
    check_h5(procs[0][1], tag)                     # rank 0's file: every dataset of the single-process file
    # ... and its bank statistics are the whole bank's, not rank 0's share (read after gkc_gather_results, which combines the ranks' counters)
    if os.path.exists(DBGINFO):
        z = np.load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
        seqs = [l for l in bytes(z["fasta"]).split(b"\n") if l and not l.startswith(b">")]
        got = info_values(procs[0][1], ("seq_number", "bank_total_nt", "seq_size_min", "seq_size_max"))
        assert got == {"seq_number": str(len(seqs)), "bank_total_nt": str(sum(len(x) for x in seqs)), "seq_size_min": str(min(len(x) for x in seqs)),
                       "seq_size_max": str(max(len(x) for x in seqs))}, got


DBGINFO = os.path.join(ROOT, "oracle", "_ref", "ref", "dbginfo")


def info_values(h5, keys):
    """first occurrence of every key in what the reference's dbginfo prints for the file"""
    info = subprocess.run([DBGINFO, "-in", h5], capture_output=True, text=True).stdout
    vals = {}
    for line in info.splitlines():
        parts = line.split(":")
        if len(parts) >= 2 and parts[0].strip() in keys and parts[0].strip() not in vals:
            vals[parts[0].strip()] = parts[1].strip()
    return vals


@needs_artefacts
@need(DBGINFO)
def test_bank_statistics_of_the_text_path(tmp_path):
    """the device-parsed text path fills BankStats from the device's counters (gkc_stats.seq_len_*): getInfo() must report the same sequence statistics as the
    iterated path, whose BankStats::update sees every Sequence (SortingCountAlgorithm.cpp:728-742, BankKmers.hpp:164-200)"""
    keys = ("bank_total_nt", "seq_number", "seq_size_min", "seq_size_max", "seq_size_mean", "seq_size_deviation", "kmers_nb_valid", "kmers_nb_invalid",
            "kmers_nb_distinct", "kmers_nb_solid")
    seen = {}
    for mode, env in (("text", None), ("iterated", {"GATB_DEVICE_NO_TEXT": "1"})):
        p, h5 = run_dbgh5("k21_default_parts", str(tmp_path), env, out_name="stats_" + mode)
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, log[-2000:]
        info = subprocess.run([DBGINFO, "-in", h5], capture_output=True, text=True).stdout
        vals = {}
        for line in info.splitlines():
            parts = line.split(":")
            if len(parts) >= 2 and parts[0].strip() in keys and parts[0].strip() not in vals:
                vals[parts[0].strip()] = parts[1].strip()
        assert set(keys) <= set(vals), (mode, vals, info[-1500:])
        seen[mode] = vals
    assert seen["text"] == seen["iterated"], seen


@needs_artefacts
@pytest.mark.parametrize("tag", ["k21_default_parts", "k21_freq_4parts"])
def test_a_bank_of_two_files_goes_to_the_device_as_text(tmp_path, tag):
    """-in a.fa,b.fa is a BankComposite of two BankFasta (Bank::open): DeviceSession::plainTextFiles walks it and both files are parsed on the device, one after
    the other; the datasets are those of the one-file run (the reads are the same, cut at a record start). The Repartitor of a composite bank: the m-mer frequencies
    (frequency order) are counted on the device over the composite's iterator, the per-bank SampleRepart loop (RepartitionAlgorithm.cpp:405-438) stays the reference's."""
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    text = bytes(z["fasta"])
    cut = text.index(b"\n>", len(text) // 2) + 1
    a, b = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    open(a, "wb").write(text[:cut]); open(b, "wb").write(text[cut:])
    extra, mem, cores = CASES[tag]
    out = str(tmp_path / "two_files")
    cmd = [EXE, "-in", a + "," + b, "-kmer-size", str(k), "-abundance-min", "2", "-out", out, "-out-tmp", str(tmp_path), "-nb-cores", cores,
           "-max-memory", mem, "-verbose", "0", "-bloom", "none", "-debloom", "none", "-branching-nodes", "none", "-no-mphf"] + extra
    r = subprocess.run(cmd, env=dict(os.environ, GATB_DEVICE_VERBOSE="1", GATB_DEVICE_REFERENCE_CONFIG="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    check_h5(out + ".h5", tag)
    log = r.stdout + r.stderr
    assert "gkc_sample_exact" not in log, log[-2000:]
    assert ("gkc_count_mmers" in log) == (tag == "k21_freq_4parts"), log[-2000:]
    if tag == "k21_freq_4parts":
        assert np.array_equal(dump_dataset(out + ".h5", "/minimizers/minimFrequency", "LE"), z["minimFrequency"])


def h5_attr(h5, path):
    import re
    out = subprocess.run([H5DUMP, "-a", path, h5], capture_output=True, text=True).stdout
    m_ = re.search(r'\(0\): "(.*?)"\s*\}', out, re.S)
    return m_.group(1) if m_ else None


def check_pipeline(h5, tag):
    """/bloom/bloom (+ its attributes), /dsk/mphf and — for the runs with dbgh5's default flags — the debloom and branching datasets, byte for byte"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    assert np.array_equal(dump_dataset(h5, "/bloom/bloom", "LE"), z["bloom"]), "/bloom/bloom differs from the unpatched reference's"
    for a in ("size", "nb_hash", "type", "kmer_size"):
        assert (h5_attr(h5, "/bloom/bloom/" + a) or "") == bytes(z["bloom_" + a]).decode(), "attribute %s of /bloom/bloom" % a
    assert np.array_equal(dump_dataset(h5, "/dsk/mphf", "LE"), z["mphf"]), "/dsk/mphf differs from the unpatched reference's"
    for name in ("debloom/bloom2", "debloom/bloom3", "debloom/bloom4", "debloom/cfp", "branching/nodes"):
        key = name.replace("/", "_")
        if key in z.files:
            assert np.array_equal(dump_dataset(h5, "/" + name, "FILE"), z[key]), "/%s differs from the unpatched reference's" % name


@needs_artefacts
@pytest.mark.parametrize("tag", sorted(PIPELINE))
@pytest.mark.parametrize("mode", ["resident", "from_storage", "single_queries", "resident_mphf_regions"])
def test_bloom_and_mphf_through_the_boundary(tmp_path, tag, mode):
    """VERDICT r3 N2 / configs[4]: BloomFactory::createBloom hands out BloomDevice<T>, BloomAlgorithm::execute and MPHFAlgorithm::execute run on the device INSIDE the
    reference's dbgh5 (integration/gatb-core.device.patch), and the file is the unpatched reference's: /dsk/solid/*, /bloom/bloom, /dsk/mphf, and with the default
    flags /debloom/* and /branching/nodes (they depend on every Bloom query the debloom step made).
      resident        the default: the solid k-mers are inserted / hashed where Stage B left them in HBM (gkc_bloom_insert_solid, gkc_mphf_build_solid, abundance map
                      on the device), the debloom step asks contains8 of a partition's k-mers in one batched device query;
      from_storage    GATB_DEVICE_NO_RESIDENT=1: the reference's BloomBuilder iterates /dsk/solid and inserts into the BloomDevice one item at a time (blocks go to the
                      device), the MPHF is built from the keys of the Iterable (gkc_mphf_build), populate() runs on the CPU;
      single_queries  GATB_DEVICE_NO_BATCHED_QUERIES=1: the debloom step's contains8 one k-mer at a time — served by the host twin, no launch per item;
      resident_mphf_regions  the default with GKC_MPHF_REGIONS_MIN=200: the MPHF levels of these small key sets are built region by region in LDS, the path key sets
                      of >= 2^21 k-mers take (csrc/gkc_mphf.hip k_mphf_region_build) — /dsk/mphf must still be the unpatched reference's bytes."""
    env = {"GATB_DEVICE_VERBOSE": "1"}
    env.update({"from_storage": {"GATB_DEVICE_NO_RESIDENT": "1"}, "single_queries": {"GATB_DEVICE_NO_BATCHED_QUERIES": "1"},
                "resident_mphf_regions": {"GKC_MPHF_REGIONS_MIN": "200"}}.get(mode, {}))
    p, h5 = run_dbgh5(tag, str(tmp_path), env, pipeline=True)
    log = p.communicate(timeout=900)[0]
    assert p.returncode == 0, log[-3000:]
    check_h5(h5, tag)
    check_pipeline(h5, tag)
    # the device really did it (the binding says so under GATB_DEVICE_VERBOSE)
    import re
    inserted = sum(int(x) for x in re.findall(r"(\d+) items inserted in blocks", log))
    queried = sum(int(x) for x in re.findall(r"(\d+) items queried in batches", log))
    if mode == "from_storage":
        assert "read from the Iterable: gkc_mphf_build" in log and "gkc_mphf_build_solid" not in log and "gkc_bloom_insert_solid" not in log, log[-3000:]
        assert inserted >= int(np.load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))["nb_solid_kmers"]), log[-3000:]
    else:
        assert "gkc_bloom_insert_solid" in log and "gkc_mphf_build_solid" in log and "gkc_mphf_abundance_map" in log, log[-3000:]
    if "defaults" in tag:                                                        # the debloom step ran: its contains8 calls
        assert (queried > 0) == (mode != "single_queries"), log[-3000:]


@needs_artefacts
@pytest.mark.parametrize("tag,fastq", [("k21_default_parts", False), ("k31_2parts_mphf", True)])
def test_gzipped_bank_goes_through_the_device_parser(tmp_path, tag, fastq):
    """a .gz FASTA / FASTQ (BankFasta.cpp:391-620 inflates inside its locked reader) is inflated by a host thread of the binding into the SAME text path as a
    plain file (DeviceSession::pushTextFiles: zlib on the prefetch thread, the device parses and scans the chunk before meanwhile); the datasets are the fixture's"""
    import gzip
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    extra, mem, cores = CASES[tag]
    text = fasta_to_fastq(bytes(z["fasta"])) if fastq else bytes(z["fasta"])
    fa = os.path.join(str(tmp_path), tag + (".fq.gz" if fastq else ".fa.gz"))
    with gzip.open(fa, "wb") as f:
        f.write(text)
    out = os.path.join(str(tmp_path), "gz")
    cmd = [EXE, "-in", fa, "-kmer-size", str(k), "-abundance-min", "2", "-out", out, "-out-tmp", str(tmp_path), "-nb-cores", cores, "-max-memory", mem, "-verbose", "0"] + COUNT_ONLY + extra
    env = dict(os.environ); env["GATB_DEVICE_REFERENCE_CONFIG"] = "1"; env["GATB_DEVICE_VERBOSE"] = "1"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "gzipped text, inflated on a host thread into the device parser" in log, log[-3000:]
    # (the bank estimate of a gzipped file differs from the plain file's — BankFasta::estimate works from the file size — and with it the Repartitor's sample: the partition
    #  LAYOUT is not the fixture's, in the unpatched reference neither; the solid records as a set and the histogram are)
    h5 = out + ".h5"
    nds = int(subprocess.run([H5DUMP, "-a", "/dsk/solid/nb_partitions", h5], capture_output=True, text=True).stdout.split('(0): "')[1].split('"')[0])
    got = []
    for p_ in range(nds):
        raw = dump_dataset(h5, "/dsk/solid/%d" % p_, "FILE"); n = len(raw) // 12; raw = raw[:n * 12].reshape(n, 12)
        got += list(zip([int.from_bytes(bytes(r_), "little") for r_ in raw[:, :8]], raw[:, 8:].copy().view("<u4")[:, 0].tolist()))
    assert sorted(got) == sorted(x for p_ in parts for x in p_)
    hist = dump_dataset(h5, "/histogram/histogram", "FILE"); hist = hist[:len(hist) // 12 * 12].reshape(-1, 12)
    assert np.array_equal(hist[:, 4:].copy().view("<u8")[:, 0], z["histogram_abundance"])


@needs_artefacts
def test_several_passes_release_the_earlier_ones(tmp_path):
    """a run of several passes must not keep the Count records of every pass in HBM (DeviceConfiguration sizes a pass for its own). The reference's Configuration
    with -max-disk 1 cuts this input into several passes (ConfigurationAlgorithm.cpp:350); the binding releases pass p - 1 when pass p begins (gkc_release_pass), nothing is
    resident at the end, BloomAlgorithm reads /dsk/solid from the storage: the SET of solid records over all nb_partitions x nb_passes datasets and /bloom/bloom are the
    one-pass fixture's."""
    tag = "k21_defaults_parts"                                                       # 6000 reads: 6 MB of k-mers, two passes at -max-disk 1
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    fa = os.path.join(str(tmp_path), tag + ".fa"); open(fa, "wb").write(bytes(z["fasta"]))
    out = os.path.join(str(tmp_path), "mp")
    cmd = [EXE, "-in", fa, "-kmer-size", str(k), "-abundance-min", "2", "-out", out, "-out-tmp", str(tmp_path), "-nb-cores", "1", "-max-memory", "2000", "-max-disk", "1", "-verbose", "0"]      # (the fixture's flags: dbgh5's defaults)
    env = dict(os.environ); env["GATB_DEVICE_REFERENCE_CONFIG"] = "1"; env["GATB_DEVICE_VERBOSE"] = "1"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    import re
    passes = {int(x) for x in re.findall(r"\[device counting\] pass (\d+),", log)}
    assert len(passes) >= 2, log[-3000:]
    assert "gkc_bloom_insert_solid" not in log, log[-3000:]                           # nothing resident after a run of several passes: inserted from the storage
    h5 = out + ".h5"
    nds = int(subprocess.run([H5DUMP, "-a", "/dsk/solid/nb_partitions", h5], capture_output=True, text=True).stdout.split('(0): "')[1].split('"')[0])
    got = []
    for p_ in range(nds):
        raw = dump_dataset(h5, "/dsk/solid/%d" % p_, "FILE"); n = len(raw) // 12; raw = raw[:n * 12].reshape(n, 12)
        got += list(zip([int.from_bytes(bytes(r_), "little") for r_ in raw[:, :8]], raw[:, 8:].copy().view("<u4")[:, 0].tolist()))
    assert sorted(got) == sorted(x for p_ in parts for x in p_)
    assert np.array_equal(dump_dataset(h5, "/bloom/bloom", "LE"), z["bloom"])


@needs_artefacts
@pytest.mark.parametrize("tag", ["k21_freq_4parts", "k21_default_parts", "k63_neighbor_mphf"])
def test_repartitor_sampling_runs_on_the_device(tmp_path, tag):
    """SURVEY 8(f)2 inside the reference: RepartitorAlgorithm's two serial iterations (RepartitionAlgorithm.cpp:348 MmersFrequency, :464 SampleRepart) are counted on the
    device (integration/gatb_device/RepartitorDevice.hpp); the tables the reference's own code builds from them are the unpatched reference's, and with
    GATB_DEVICE_NO_REPARTITOR=1 the functors run instead: the same tables."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    freq = "-minimizer-type" in CASES[tag][0]
    tables = []
    for how, env in (("device", {"GATB_DEVICE_VERBOSE": "1"}), ("functors", {"GATB_DEVICE_VERBOSE": "1", "GATB_DEVICE_NO_REPARTITOR": "1"})):
        p, h5 = run_dbgh5(tag, str(tmp_path), env, out_name=how)
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, log[-2000:]
        assert ("gkc_sample_exact" in log) == (how == "device"), log[-3000:]
        assert ("gkc_count_mmers" in log) == (how == "device" and freq), log[-3000:]
        check_h5(h5, tag)
        tables.append(dump_dataset(h5, "/minimizers/minimRepart", "LE"))
        if freq:
            f = dump_dataset(h5, "/minimizers/minimFrequency", "LE")
            assert np.array_equal(f, z["minimFrequency"]), "minimFrequency differs from the unpatched reference's"
    assert np.array_equal(tables[0], tables[1])


REF_DBGH5 = os.path.join(ROOT, "oracle", "_ref", "ref", "dbgh5")


@needs_artefacts
@need(REF_DBGH5)
@pytest.mark.parametrize("freq", [False, True])
def test_repartitor_stop_rules_against_the_unpatched_reference(tmp_path, freq):
    """The sample sizes only bite on a bank larger than the fixtures: SampleRepart stops in the sequence where more than max(5 % of the sequences, 10^6) super-k-mers have been
    seen (RepartitionAlgorithm.cpp:451, :205-212), MmersFrequency after 5 % of the sequences + 1 (:322, :113-117). 2.5e5 reads of 150 bp hold 2.7e6 super-k-mers: the
    unpatched reference run HERE on the same file is the expectation for /minimizers/minimRepart and minimFrequency."""
    rng = np.random.default_rng(20250930)
    G, n, L = 2_000_000, 250_000, 150
    genome = rng.integers(0, 4, G).astype(np.uint8)
    start = rng.integers(0, G - L, n)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[genome[start[:, None] + np.arange(L)[None, :]]]
    bases[rng.random((n, L)) < 0.002] = ord("N")                                  # (some sequences lose k-mers and super-k-mers to N)
    rec = np.empty((n, L + 4), dtype=np.uint8); rec[:, 0] = ord(">"); rec[:, 1] = ord("r"); rec[:, 2] = 10; rec[:, 3:3 + L] = bases; rec[:, 3 + L] = 10
    fa = os.path.join(str(tmp_path), "reads.fa"); rec.tofile(fa)
    flags = ["-kmer-size", "31", "-abundance-min", "2", "-out-tmp", str(tmp_path), "-nb-cores", "8", "-max-memory", "200", "-verbose", "0"] + COUNT_ONLY
    flags += ["-minimizer-type", "1", "-repartition-type", "1"] if freq else []
    env = dict(os.environ); env["GATB_DEVICE_REFERENCE_CONFIG"] = "1"; env["GATB_DEVICE_VERBOSE"] = "1"
    out = {}
    for name, exe in (("ref", REF_DBGH5), ("dev", EXE)):
        o = os.path.join(str(tmp_path), name)
        r = subprocess.run([exe, "-in", fa, "-out", o] + flags, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out[name] = (o + ".h5", r.stdout + r.stderr)
    log = out["dev"][1]
    assert "gkc_sample_exact" in log and ("gkc_count_mmers" in log) == freq, log[-3000:]
    import re
    sampled = int(re.search(r"(\d+) super-k-mers of the first (\d+) sequences sampled", log).group(1))
    assert 1_000_000 < sampled < 1_000_000 + 64, sampled                               # stopped in the sequence that crossed the threshold, not at the end of the bank
    a = dump_dataset(out["ref"][0], "/minimizers/minimRepart", "LE"); b = dump_dataset(out["dev"][0], "/minimizers/minimRepart", "LE")
    assert len(a) > 2 * 4 ** 10 and int(a[:2].copy().view("<u2")[0]) > 1                  # (Repartitor::save: the number of partitions first — several: the table says something)
    assert np.array_equal(a, b), "minimRepart differs from the unpatched reference's"
    if freq:
        assert np.array_equal(dump_dataset(out["ref"][0], "/minimizers/minimFrequency", "LE"), dump_dataset(out["dev"][0], "/minimizers/minimFrequency", "LE"))
    for ds in ("/histogram/histogram",):
        assert np.array_equal(dump_dataset(out["ref"][0], ds, "FILE"), dump_dataset(out["dev"][0], ds, "FILE"))


UNITIGS = os.path.join(ROOT, "oracle", "_ref", "unitigs_check")            # GraphUnitigs linked WITH the patched units: counts on the device
UNITIGS_REF = os.path.join(ROOT, "oracle", "_ref", "ref", "unitigs_check")  # GraphUnitigs of the unpatched library: the consumer of an .h5


def canonical_unitigs(fa):
    import hashlib
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for line in open(fa, "rb"):
        if not line.startswith(b">"):
            s_ = line.strip(); seqs.append(min(s_, s_.translate(comp)[::-1]))
    seqs.sort()
    return [len(seqs), sum(len(x) for x in seqs), hashlib.sha256(b"\n".join(seqs)).hexdigest()]


@needs_artefacts
@need(UNITIGS, UNITIGS_REF)
def test_graphunitigs_consumes_the_device_output(tmp_path):
    """north_star: "drops into GraphUnitigs/dbgh5 unchanged" (VERDICT r3 N1). (a) the .h5 the patched dbgh5 wrote on the MI355X in the mode GraphUnitigs forces
    (frequency-order minimizers, 4 partitions) is opened by the UNPATCHED reference's GraphUnitigs (restart path, GraphUnitigs.cpp:907-944); (b) GraphUnitigs linked with
    the patched units counts the FASTA itself on the device (GraphUnitigs.cpp:222). Both must give the unitig set the reference gives
    (tests/golden/reference_run/k21_freq_4parts_unitigs.json: count, total length, sha256 of the sorted canonical sequences)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_run", "k21_freq_4parts_unitigs.json")))
    want = [want["unitigs"], want["total_length"], want["sha256_sorted_canonical"]]
    p, h5 = run_dbgh5("k21_freq_4parts", str(tmp_path))
    log = p.communicate(timeout=600)[0]
    assert p.returncode == 0, log[-2000:]
    r = subprocess.run([UNITIGS_REF, h5, str(tmp_path / "from_h5"), "1"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert canonical_unitigs(str(tmp_path / "from_h5.unitigs.fa")) == want
    fa = str(tmp_path / "k21_freq_4parts.fa")
    r = subprocess.run([UNITIGS, fa, str(tmp_path / "from_fa"), "1", "-kmer-size", "21", "-abundance-min", "2", "-out-tmp", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=dict(os.environ, GATB_DEVICE_VERBOSE="1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "[device counting]" in r.stderr, r.stderr[-2000:]                   # the count inside GraphUnitigs ran on the device
    assert canonical_unitigs(str(tmp_path / "from_fa.unitigs.fa")) == want


@needs_artefacts
@need(DBGINFO)
def test_device_time_keys_in_getinfo(tmp_path):
    """getInfo() of the patched SortingCountAlgorithm carries the device's figures where the reference's commands put 1.read / 2.sort / 3.dump
    (fillsolid_time, SortingCountAlgorithm.cpp:777-780): device_stage_a / device_stage_b / device_wait / device_hand_over, stored in the .h5's xml"""
    p, h5 = run_dbgh5("k21_default_parts", str(tmp_path))
    log = p.communicate(timeout=600)[0]
    assert p.returncode == 0, log[-2000:]
    info = subprocess.run([DBGINFO, "-in", h5], capture_output=True, text=True).stdout
    for key in ("fillsolid_time", "device_stage_a", "device_stage_b", "device_wait", "device_hand_over"):
        assert key in info, (key, info[-2500:])


@needs_artefacts
@pytest.mark.parametrize("tag", ["k21_default_parts", "k31_2parts_mphf", "k63_neighbor_mphf"])
def test_configuration_sized_from_the_device(tmp_path, tag):
    """SURVEY 8(f)4 / VERDICT r3 Missing #2: in the patched dbgh5 ConfigurationAlgorithm sizes partitions and passes from the HBM of the device
    (integration/gatb_device/DeviceConfiguration.hpp) instead of host RAM and disk: whatever -max-memory says, these small inputs become ONE partition in one pass
    (the fixtures' reference runs cut them into 4 / 2 / 1) — and the solid k-mers with their counts are the same set."""
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    p, h5 = run_dbgh5(tag, str(tmp_path), {"GATB_DEVICE_REFERENCE_CONFIG": "0", "GATB_DEVICE_VERBOSE": "1"})
    log = p.communicate(timeout=600)[0]
    assert p.returncode == 0, log[-2000:]
    assert "[device configuration]" in log and "1 pass(es), 1 partitions" in log, log[-2000:]
    assert h5_attr(h5, "/dsk/solid/nb_partitions") == "1"
    rec = 12 if k <= 31 else 20
    raw = dump_dataset(h5, "/dsk/solid/0", "FILE")
    n = len(raw) // rec; raw = raw[:n * rec].reshape(n, rec)
    got = list(zip([int.from_bytes(bytes(r), "little") for r in raw[:, :rec - 4]], raw[:, rec - 4:].copy().view("<u4")[:, 0].tolist()))
    assert got == sorted(x for part in parts for x in part)                     # ascending in the one dataset, same k-mers, same counts


@needs_artefacts
def test_text_the_device_parser_refuses_goes_through_the_iterated_bank(tmp_path):
    """A multi-line FASTQ (sequence and quality wrapped over two lines each) is what the reference's reader takes (BankFasta.cpp:488-571) and the device parser refuses
    (GKC_ERR_FORMAT: not expressible line by line): DeviceSession::pushTextFiles gives up, the pass starts again with the bank iterated, the datasets are the fixture's.
    Run with -verbose 1: the progress the text path had reported is owed to the listener, never wound back (a negative increment would spin in Progress::inc)."""
    tag = "k21_default_parts"
    z, k, m, nbpart, table, parts = load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    recs, name, seq = [], None, []
    def flush():
        if name is not None:
            sq = b"".join(seq); h = len(sq) // 2
            recs.append(b"@" + name + b"\n" + sq[:h] + b"\n" + sq[h:] + b"\n+\n" + b"I" * h + b"\n" + b"I" * (len(sq) - h) + b"\n")
    for line in bytes(z["fasta"]).split(b"\n"):
        if line.startswith(b">"):
            flush(); name = line[1:]; seq = []
        elif line:
            seq.append(line.strip())
    flush()
    fq = str(tmp_path / "wrapped.fq"); open(fq, "wb").write(b"".join(recs))
    extra, mem, cores = CASES[tag]
    out = str(tmp_path / "wrapped")
    cmd = [EXE, "-in", fq, "-kmer-size", str(k), "-abundance-min", "2", "-out", out, "-out-tmp", str(tmp_path), "-nb-cores", "4", "-max-memory", mem, "-verbose", "1"] + COUNT_ONLY + extra
    r = subprocess.run(cmd, env=dict(os.environ, GATB_DEVICE_VERBOSE="1", GATB_DEVICE_REFERENCE_CONFIG="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "device counting" in r.stderr
    z2 = np.load(os.path.join(ROOT, "tests", "golden", "reference_run", tag + ".npz"))
    rec = 12
    got = []
    for p_ in range(int(h5_attr(out + ".h5", "/dsk/solid/nb_partitions"))):
        raw = dump_dataset(out + ".h5", "/dsk/solid/%d" % p_, "FILE"); n = len(raw) // rec; raw = raw[:n * rec].reshape(n, rec)
        got += list(zip([int.from_bytes(bytes(x), "little") for x in raw[:, :8]], raw[:, 8:].copy().view("<u4")[:, 0].tolist()))
    assert sorted(got) == sorted(x for part in parts for x in part)            # (-nb-cores 4: the reference's Configuration may cut other partitions; the k-mers and counts are the fixture's)
