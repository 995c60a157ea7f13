"""The toolkit's read simulator (bin/createSimulatedPARCLIPDataset.pl) restated in plain Python, rule for rule and in the
Perl's order, with the library's random stream in place of Math::Random (include/parasuite_hip.h, ps_simulate_reads, has
the rules and the stream in words).  One transcript after the other, one cluster after the other, one read after the other:
nothing here is arranged the way the device code is.  ps_simulate_reads must give these bytes.

simulate(fasta, error_profile, site_frequency, site_positions, qualities, indels, bound_prob, seed, ...) takes the CONTENTS of
the six input files as bytes and returns ({".fastq": bytes, ".clusters": ..., "_snps.vsf": ..., ".log": ..., ".err": ...},
stats); SimError where the library reports an error."""
import re

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SELECT_READ, SNP_RATE, SNP_REPORT = 0.216, 0.01, 0.8
MAX_LENGTH, MIN_LENGTH = 30, 7
ACGT = "ACGT"
OTHERS = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}              # mutate_base's tables

# slots of a cluster's unit (cluster ordinal 1..3, read ordinal 0)
C_NREADS, C_POS, C_NT2C, C_NSTART, C_NEND, C_STARTS, C_ENDS, C_BOUND, C_SITE, C_SNP = 0, 12, 13, 14, 15, 16, 52, 88, 89, 128
# slots of a transcript's unit (cluster ordinal 0, read ordinal 0)
T_SELECT, T_NCLUSTERS = 0, 1
# slots of a read's unit (cluster ordinal 1..3, read ordinal i + 1); the per-base loop: R_LOOP + 64 * iteration + ...
R_START, R_END, R_LOOP = 0, 1, 16
L_TEST, L_ANYBASE, L_SNP, L_INDEL, L_INSBASE, L_QUAL, L_QUAL_SNP, L_QUAL_INS = 0, 1, 2, 3, 4, 8, 20, 32


class SimError(Exception):
    pass


def mix(x):
    """the finalizer of splitmix64"""
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ x >> 31


def run_key(seed):
    return mix((seed + GOLDEN) & M64)


def unit_key(run, transcript, cluster, read):
    return mix(mix(run ^ transcript) ^ (cluster << 32 | read))


def draw32(unit, slot):
    return mix(unit ^ slot) >> 32


def normal_from_draws(draws, mean, sd):
    """random_normal: twelve uniforms; their sum is exact, the product and the sum round once each"""
    assert len(draws) == 12
    z = float(sum(draws) - 6 * (1 << 32)) * 2.0 ** -32
    return mean + sd * z


def normal(unit, slot, mean, sd):
    return normal_from_draws([draw32(unit, slot + i) for i in range(12)], mean, sd)


def ceil_rand(unit, slot, k):
    """ceil(rand() * k) taken as 1 + floor(u * k), in integers; k <= 0 gives 0 (the Perl's value is <= 0 there: the cluster is skipped)"""
    return 1 + (draw32(unit, slot) * k >> 32) if k > 0 else 0


def floor_rand(unit, slot, k):
    return draw32(unit, slot) * k >> 32


def rand(unit, slot):
    return draw32(unit, slot) * 2.0 ** -32


_NUM = re.compile(r"[ \t\n\r\f\v]*([+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)")


def perl_num(s):
    """a string in numeric context: the decimal number it starts with, 0 without one (a "\\r" behind it is not looked at)"""
    m = _NUM.match(s)
    return float(m.group(1)) if m else 0.0


def _lines(data):
    """<FH> and chomp: lines end at "\\n" only; a last line without one counts"""
    text = data.decode("latin-1")
    out = text.split("\n")
    if out and out[-1] == "":
        out.pop()
    return out


def _split_ws(line):
    """split('\\s+', line): a leading empty field stays, trailing ones are dropped"""
    f = re.split(r"[ \t\n\r\f\v]+", line)
    while f and f[-1] == "":
        f.pop()
    return f


def _field(f, k):
    return perl_num(f[k]) if k < len(f) else 0.0


def load_profiles(error_profile, site_frequency, site_positions, qualities, indels, allow_indels=True):
    rows = _lines(error_profile)
    if len(rows) < 4:
        raise SimError("the error profile has %d lines, 4 are needed" % len(rows))
    thr = []                                                             # per base: the three thresholds of the error step
    for run in range(4):
        f = _split_ws(rows[run])
        v = [_field(f, k) for k in range(4)]
        no_error = v[(run + 1) % 4] + v[(run + 2) % 4] + v[(run + 3) % 4]
        v[run] = 1 - no_error
        t0 = v[run]
        t1 = t0 + v[(run + 1) % 4]
        thr.append((t0, t1, t1 + v[(run + 2) % 4]))
    freq = [perl_num(l) for l in _lines(site_frequency)]
    if len(freq) < 4:
        raise SimError("the site frequency file has %d lines, 4 are needed" % len(freq))
    pos = [perl_num(l) for l in _lines(site_positions)]
    if len(pos) < 40:
        raise SimError("the site positions file has %d lines, 40 are needed" % len(pos))
    q = []
    for l in _lines(qualities):
        f = l.split("\t")
        while f and f[-1] == "":
            f.pop()
        q.append((_field(f, 0), _field(f, 1)))
    if len(q) < 31:
        raise SimError("the quality file has %d lines, 31 are needed" % len(q))
    ind = []
    if allow_indels:
        for l in _lines(indels):
            f = _split_ws(l)
            ind.append((_field(f, 0), _field(f, 1)))
        if len(ind) < 31:
            raise SimError("the indel profile has %d lines, 31 are needed" % len(ind))
    return thr, freq, pos, q, ind


def read_fasta(data):
    """(header, sequence) per '>' line; text before the first header is dropped; "\\r" stays where a CRLF file has it"""
    out, header, seq = [], None, []
    for line in _lines(data):
        if line.startswith(">"):
            if header is not None:
                out.append((header, "".join(seq)))
            header, seq = line, []
        elif header is not None:
            seq.append(line)
    if header is not None:
        out.append((header, "".join(seq)))
    return out


_INT = re.compile(r"[+-]?[0-9]{1,18}\Z")


def parse_header(header, seq_len):
    """-> (fields, chromosome, exon starts, exon ends, strand); the genomic position list is never built: gp() reads it off"""
    f = header.split("|")
    while f and f[-1] == "":
        f.pop()
    name = header[1:]
    if len(f) < 6:
        raise SimError("transcript %s: the header has %d '|' fields, 6 are needed" % (name, len(f)))

    def bounds(text):
        p = text.split(";")
        while p and p[-1] == "":
            p.pop()
        for v in p:
            if not _INT.match(v):
                raise SimError("transcript %s: exon bound '%s' is not an integer" % (name, v))
        return sorted(int(v) for v in p)
    starts, ends = bounds(f[3]), bounds(f[4])
    if len(starts) != len(ends) or not starts:
        raise SimError("transcript %s: %d exon starts and %d exon ends" % (name, len(starts), len(ends)))
    total = sum(max(0, e - s + 1) for s, e in zip(starts, ends))
    if total < seq_len:
        raise SimError("transcript %s: the exons hold %d positions, the sequence has %d" % (name, total, seq_len))
    return f, f[2], starts, ends, perl_num(f[-1])


def gp(starts, ends, strand, idx):
    """$genomic_positions[idx]"""
    lens = [max(0, e - s + 1) for s, e in zip(starts, ends)]
    if strand == -1:
        idx = sum(lens) - 1 - idx
    for s, n in zip(starts, lens):
        if idx < n:
            return s + idx
        idx -= n
    raise AssertionError("position outside the exons")


def perl_str(x):
    """a number as Perl prints it"""
    return "%.15g" % x


def quality(unit, slot, mean, sd):
    v = normal(unit, slot, mean, sd)
    q = 64 if v >= 65.0 else (3 if v < 3.0 else int(v))                  # int(v) > 64 -> 64; int(v) <= 2 -> 3
    return chr(33 + q)


def simulate(fasta, error_profile, site_frequency, site_positions, qualities, indels, bound_prob, seed,
             select_read=None, snp_rate=None, snp_report=None, allow_indels=None):
    select_read = SELECT_READ if select_read is None or select_read <= 0 else select_read
    snp_rate = SNP_RATE if snp_rate is None or snp_rate < 0 else snp_rate
    snp_report = SNP_REPORT if snp_report is None or snp_report < 0 else snp_report
    allow_indels = True if allow_indels is None or allow_indels < 0 else bool(allow_indels)
    thr, freq, sitepos, qual, ind = load_profiles(error_profile, site_frequency, site_positions, qualities, indels, allow_indels)
    transcripts = read_fasta(fasta)
    run = run_key(seed)
    fastq, clusters_out, vsf, err = [], [], ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"], []
    st = dict.fromkeys(("n_reads", "n_bases_simulated", "sum_read_length", "n_clusters", "n_t2c", "n_errors", "most_t2c",
                        "most_errors", "n_indels", "n_snps", "n_selected", "n_clusters_skipped", "n_reads_skipped",
                        "n_snps_reported", "n_non_acgt", "n_snps_preselected", "n_snp_positions"), 0)
    st["n_transcripts"] = len(transcripts)
    clusters_passed, snp_id = 0, 1

    for t, (header, seq) in enumerate(transcripts[:-1]):                 # the last one is never simulated
        fields, chrom, starts, ends, strand = parse_header(header, len(seq))
        L = len(seq)
        tu = unit_key(run, t, 0, 0)
        if not rand(tu, T_SELECT) < select_read:
            continue
        st["n_selected"] += 1
        num_clusters = ceil_rand(tu, T_NCLUSTERS, 3)
        st["n_clusters"] += num_clusters
        cluster_index = 1
        for c in range(1, num_clusters + 1):
            cu = unit_key(run, t, c, 0)
            n_reads = int(normal(cu, C_NREADS, 16.0, 10.0))
            clusters_passed += 1
            cluster_pos = ceil_rand(cu, C_POS, L - MAX_LENGTH)
            if cluster_pos < 10 or L - cluster_pos < MAX_LENGTH:
                st["n_clusters_skipped"] += 1
                continue
            num_t2c = ceil_rand(cu, C_NT2C, 4)
            num_start = ceil_rand(cu, C_NSTART, 3)
            num_end = ceil_rand(cu, C_NEND, 3)
            start_pos = [int(normal(cu, C_STARTS + 12 * i, float(cluster_pos), 1.0)) for i in range(num_start)]
            end_pos = [int(normal(cu, C_ENDS + 12 * i, float(cluster_pos + (MAX_LENGTH - MIN_LENGTH)), 1.0)) for i in range(num_end)]
            cl_start, cl_end = gp(starts, ends, strand, min(start_pos)), gp(starts, ends, strand, max(end_pos))
            if strand == -1:
                cl_start, cl_end = cl_end, cl_start
            assert max(end_pos) < L                                      # twelve uniforms keep an end within pos + 29 <= L - 1
            bound, sites = 0, {}
            if rand(cu, C_BOUND) < bound_prob:
                bound = 1
                tpos = [k for k in range(max(start_pos), min(end_pos)) if seq[k] == "T"]
                for k in range(num_t2c):
                    if not tpos:
                        break
                    if len(tpos) == 1:
                        pick = 0
                    else:                                                # get_t2c_position
                        shift = max(start_pos)
                        total = 0.0
                        for p in tpos:
                            total += sitepos[p - shift]
                        r = rand(cu, C_SITE + k) * total
                        done, pick = 0.0, -1
                        for i, p in enumerate(tpos):
                            done += sitepos[p - shift]
                            if r <= done:
                                pick = i
                                break
                    sites[tpos[pick]] = freq[k]
                    del tpos[pick]
            clusters_out.append("cl_%d\tchr%s\t%d\t%d\t%d\n" % (clusters_passed, chrom, cl_start, cl_end, bound))

            snps = {}                                                    # the whole transcript, once per cluster
            st["n_snp_positions"] += L
            for z in range(L):
                if not rand(cu, C_SNP + 4 * z) <= snp_rate:
                    continue
                ref = seq[z]
                alt = OTHERS[ref][floor_rand(cu, C_SNP + 4 * z + 1, 3)] if ref in OTHERS else ""
                snps[z] = (1.0 if rand(cu, C_SNP + 4 * z + 2) <= 0.5 else 0.5, alt)
                if rand(cu, C_SNP + 4 * z + 3) <= snp_report:
                    vsf.append("%s\t%d\tsnp%d\t%s\t%s\t.\t.\t.\n" % (chrom, gp(starts, ends, strand, z), snp_id, ref, alt))
                    st["n_snps_reported"] += 1
                snp_id += 1
                st["n_snps_preselected"] += 1

            for i in range(n_reads):
                ru = unit_key(run, t, c, i + 1)
                start = start_pos[floor_rand(ru, R_START, num_start)]
                end = end_pos[floor_rand(ru, R_END, num_end)]
                if end - start > MAX_LENGTH or start >= end:
                    st["n_reads_skipped"] += 1
                    continue
                wt = seq[start:end]
                out_seq, out_qual = [], []
                num_t2c_read = num_error = 0
                indel_set = False
                st["sum_read_length"] += len(wt)
                j, it = 0, 0
                while j < len(wt):
                    base = R_LOOP + 64 * it
                    it += 1
                    q_mean, q_sd = qual[j]
                    cur = wt[j]
                    test = rand(ru, base + L_TEST)
                    if bound and start + j in sites:
                        if sites[start + j] > test:
                            out_seq.append("C")
                            st["n_t2c"] += 1
                            num_t2c_read += 1
                        else:
                            out_seq.append(cur)
                        out_qual.append(quality(ru, base + L_QUAL, q_mean, q_sd))
                        j += 1
                        continue
                    if cur in ACGT:
                        row, here = ACGT.index(cur), ACGT.index(cur)
                    else:
                        err.append("unrecognized base in ACGT_hash=%s\nSequence_header=%s\nSequence=%s\n" % (cur, header, seq))
                        st["n_non_acgt"] += 1
                        row, here = floor_rand(ru, base + L_ANYBASE, 4), 0
                    if start + j in snps:
                        if rand(ru, base + L_SNP) <= snps[start + j][0]:
                            out_qual.append(quality(ru, base + L_QUAL_SNP, q_mean, q_sd))
                            out_seq.append(snps[start + j][1])
                            st["n_snps"] += 1
                    out_qual.append(quality(ru, base + L_QUAL, q_mean, q_sd))
                    t0, t1, t2 = thr[row]
                    if not test < t0:
                        k = 1 if test < t1 else (2 if test < t2 else 3)
                        out_seq.append(ACGT[(here + k) % 4])
                        st["n_errors"] += 1
                        num_error += 1
                        if k == 2:
                            num_t2c_read += 1                            # the Perl's count, :538
                        j += 1
                        continue
                    out_seq.append(cur)
                    if allow_indels:
                        test_indel = rand(ru, base + L_INDEL)
                        if not indel_set and test_indel <= ind[j][0]:
                            out_qual.append(quality(ru, base + L_QUAL_INS, q_mean, q_sd))
                            out_seq.append(ACGT[floor_rand(ru, base + L_INSBASE, 4)])
                            st["n_indels"] += 1
                            indel_set = True
                            continue                                     # position j again
                        if not indel_set and test_indel <= ind[j][1]:
                            st["n_indels"] += 1
                            indel_set = True
                            j += 1
                            continue
                    st["n_bases_simulated"] += 1
                    j += 1
                st["most_t2c"] = max(st["most_t2c"], num_t2c_read)
                st["most_errors"] = max(st["most_errors"], num_error)
                if strand == 1:
                    r_start, r_end = gp(starts, ends, strand, start), gp(starts, ends, strand, end)
                else:
                    r_start, r_end = gp(starts, ends, strand, end) + 1, gp(starts, ends, strand, start) + 1
                fastq.append("@SEQ_ID:%s|%s|%s|%d|%d|%d-%d:%d\n%s\n+\n%s\n" % (fields[0], fields[1], chrom, r_start, r_end, bound,
                                                                              cluster_index, i, "".join(out_seq), "".join(out_qual)))
                st["n_reads"] += 1
            cluster_index += 1

    if st["n_reads"] == 0:
        raise SimError("no read was drawn")
    st["avg_read_length"] = st["sum_read_length"] / st["n_reads"]
    st["avg_reads_per_cluster"] = st["n_reads"] / st["n_clusters"]
    log = ("number reads generated: %d\nnumber bases simulated: %d\naverage read-length: %s\nnumber clusters generated: %d\n"
           "average reads per cluster: %s\nT2C mutations occured: %d\nsequencing errors occured: %d\nread with most T2C: %d\n"
           "read with most errors: %d\nnumber indels generated: %d\nnumer snps generated: %d\n"
           "\nSome parameters:\nselect_prob=%s\nread bound by RBP probability: %s\n"
           % (st["n_reads"], st["n_bases_simulated"], perl_str(st["avg_read_length"]), st["n_clusters"],
              perl_str(st["avg_reads_per_cluster"]), st["n_t2c"], st["n_errors"], st["most_t2c"], st["most_errors"], st["n_indels"],
              st["n_snps"], perl_str(select_read), perl_str(bound_prob)))
    files = {".fastq": "".join(fastq), ".clusters": "".join(clusters_out), "_snps.vsf": "".join(vsf), ".log": log, ".err": "".join(err)}
    return {k: v.encode("latin-1") for k, v in files.items()}, st


INT_KEYS = ("n_reads", "n_bases_simulated", "sum_read_length", "n_clusters", "n_t2c", "n_errors", "most_t2c", "most_errors", "n_indels",
            "n_snps", "n_transcripts", "n_selected", "n_clusters_skipped", "n_reads_skipped", "n_snps_reported", "n_non_acgt",
            "n_snps_preselected", "n_snp_positions")
