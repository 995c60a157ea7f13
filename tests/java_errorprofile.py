"""Plain-Python restatement of ErrorProfiling.inferErrorProfile (ErrorProfiling.java:145-591) for all six files it writes,
with this library's documented deviations where the Java throws (include/parasuite_hip.h, ps_error_profile_full):

  - qualities are booked for read positions i < len(QUAL) only (the Java reads QUAL[i] for every i < width and fails past
    the read on deletion and N records);
  - a .qualityPerMismatch pair whose QUAL index lies past the read (reverse-strand N records) is left out and counted;
  - a record with QUAL '*' adds nothing to the two quality files and is counted;
  - sums are exact (Python integers), where the Java's qualityPerMismatch is a 32-bit int.

Small inputs only: one Python loop per record and base.  SAM text in, the bytes of each file out.  Reference bases come
from the caller's FASTA; Double.toString is the oracle's port (orc.java_double).  Test infrastructure, not product code."""
import math

import orc

FILES = (".errorprofile", ".indelprofile", ".errorprofile.vcf", ".qualityPerMismatch", ".indels", ".qualities")
_CODE = {ord(c): i for i, c in enumerate("ACGT")}
_CODE.update({ord(c): i for i, c in enumerate("acgt")})
_COMP = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}


def read_fasta(path):
    """{first word of the header: sequence bytes}"""
    seqs, name, parts = {}, None, []
    for line in open(path, "rb"):
        line = line.rstrip(b"\r\n")
        if line.startswith(b">"):
            if name is not None:
                seqs[name] = b"".join(parts)
            name, parts = line[1:].split()[0].decode(), []
        else:
            parts.append(line)
    if name is not None:
        seqs[name] = b"".join(parts)
    return seqs


def _cigar(s):
    ops, n = [], 0
    for ch in s:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            ops.append((ch, n))
            n = 0
    return ops


def _pos(b):                                   # calculateArrayPos, :634-664
    return _CODE.get(b, -1)


def _revcomp(a):                               # htsjdk SequenceUtil.reverseComplement: other bytes keep their value
    return bytearray(_COMP.get(b, b) for b in reversed(a))


def infer(sam_text, ref, max_read_len, infer_qualities):
    """(files, stats): files maps each suffix of FILES to the bytes the library writes; ref = read_fasta(...)"""
    c = counts(sam_text, ref, max_read_len, infer_qualities)
    return render(c, max_read_len, infer_qualities), c["st"]


def counts(sam_text, ref, max_read_len, infer_qualities):
    """the counting loop (:145-409): everything the six files are written from, as a dict.  All of it but the quality
    lists is a sum over the records, so the counts of a concatenation are the sums of its parts' counts"""
    ML = max_read_len
    conv = [[[0] * 4 for _ in range(4)] for _ in range(ML)]
    ins, dele = [0.0] * ML, [0.0] * ML
    qpm_sum, qpm_cnt = [[0] * 4 for _ in range(4)], [[0] * 4 for _ in range(4)]
    qlists = [[] for _ in range(ML)]
    st = dict(n_records=0, n_counted=0, n_unmapped=0, n_duplicate=0, n_start_zero=0, n_indel_reads=0, n_skipped=0,
              n_without_qual=0, n_qual_beyond_read=0)
    for line in sam_text.split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        st["n_records"] += 1
        flag, rname, pos, cig = int(f[1]), f[2], int(f[3]), f[5]
        if flag & 4:
            st["n_unmapped"] += 1
            continue
        if flag & 1024:
            st["n_duplicate"] += 1
            continue
        if pos == 0:
            st["n_start_zero"] += 1
            continue
        read = bytearray(b"" if f[9] == "*" else f[9].encode())
        quals = None if f[10] == "*" else [ord(c) - 33 for c in f[10]]
        ops = _cigar(cig) if cig != "*" else []
        span = sum(n for o, n in ops if o in "MDN=X")
        end = pos + span - 1 if span > 0 else pos                            # htsjdk getAlignmentEnd
        refs = bytearray(ref[rname][pos - 1:end])
        st["n_counted"] += 1
        L, R = len(read), len(refs)
        width = max(L, R)
        if width > ML:
            raise ValueError("a read (or its reference span) is longer than the maximum read length")
        skip = False
        if L != R:                                                           # :194-293
            rt, dt = bytearray(width), bytearray(width)
            pm = pref = prd = 0
            for o, n in ops:
                if o in "MX=":
                    for z in range(n):
                        if z + pm >= width or z + pref >= R:
                            skip = True
                            continue
                        rt[z + pm] = refs[z + pref]
                        if z + prd >= L:
                            skip = True
                            continue
                        dt[z + pm] = read[z + prd]
                    pm += n
                    pref += n
                    prd += n
                elif o == "N":
                    pref += n
                    prd += n
                elif o == "I":
                    for z in range(n):
                        if pm + z < width:
                            rt[pm + z] = 45
                    pm += n
                    prd += n
                    for q in range(1, n + 1):
                        if pm + q < ML:
                            ins[pm + q] += 1.0
                elif o == "D":
                    for z in range(n):
                        if pm + z < width:
                            dt[pm + z] = 45
                    pm += n
                    pref += n
                    for q in range(1, n + 1):
                        if pm + q < ML:
                            dele[pm + q] += 1.0
            st["n_indel_reads"] += 1
            refs, read = rt, dt
        if skip:
            st["n_skipped"] += 1
            continue
        if flag & 16:                                                        # :311-316; QUAL stays as it is (:301)
            read, refs = _revcomp(read), _revcomp(refs)
        has_q = quals is not None and L > 0
        if not has_q:
            st["n_without_qual"] += 1
        gapped = "I" in cig or "D" in cig
        for i in range(width):
            pr, pd = _pos(refs[i]), _pos(read[i])
            if pr >= 0 and pd >= 0:
                conv[i][pr][pd] += 1
                if has_q and not gapped:
                    if i < len(quals):
                        qpm_sum[pr][pd] += quals[i]
                        qpm_cnt[pr][pd] += 1
                    else:
                        st["n_qual_beyond_read"] += 1
            if infer_qualities and has_q and i < len(quals):
                qlists[i].append(quals[i])
    return dict(conv=conv, ins=ins, dele=dele, qpm_sum=qpm_sum, qpm_cnt=qpm_cnt, qlists=qlists, st=st)


def render(c, max_read_len, infer_qualities):
    """the six files (:421-591) of the counts"""
    ML = max_read_len
    conv, ins, dele, qpm_sum, qpm_cnt, qlists = (c[k] for k in ("conv", "ins", "dele", "qpm_sum", "qpm_cnt", "qlists"))
    jd = orc.java_double
    tot, base, per_pos = [[0.0] * 4 for _ in range(4)], [0.0] * 4, [0.0] * ML
    for i in range(ML):
        for j in range(4):
            for k in range(4):
                x = float(conv[i][j][k])
                tot[j][k] += x
                base[j] += x
                per_pos[i] += x
    div = lambda a, b: a / b if b != 0 else (math.nan if a == 0 else math.copysign(math.inf, a))
    ep = vcf = qpm = ""
    for j in range(4):
        for k in range(4):
            vcf += "ACGT"[j] + "\t" + "ACGT"[k] + "\t" + jd(tot[j][k]) + "\n"
            ep += jd(div(tot[j][k], base[j])) + "\t"
            qpm += jd(div(float(qpm_sum[j][k]), float(qpm_cnt[j][k]))) + "\t"
        ep += "\n"
        qpm += "\n"
        vcf += "\n"
    ins_all = del_all = 0.0
    ins_zero = del_zero = 0
    indels = ""
    for i in range(ML):                                                      # :549-579
        if per_pos[i] == 0.0:
            x = y = 0.0
            ins_zero += 1
            del_zero += 1
        else:
            x, y = ins[i] / per_pos[i], dele[i] / per_pos[i]
            if x > 0:
                ins_all += x
            else:
                ins_zero += 1
            if y > 0:
                del_all += y
            else:
                del_zero += 1
        indels += jd(x) + "\t" + jd(y) + "\n"
    if ML == ins_zero and ML == del_zero:
        ins_all = del_all = 0.0
    else:
        ins_all, del_all = div(ins_all, float(ML - ins_zero)), div(del_all, float(ML - del_zero))
    qualities = ""
    if infer_qualities:                                                      # :421-436
        for i in range(ML):
            vals, n = qlists[i], float(len(qlists[i]))
            mean = div(float(sum(vals)), n)
            ssd = 0.0
            for v in vals:                                                   # file order, one rounded add at a time
                d = v - mean
                ssd += d * d                                                 # Math.pow(d, 2.0) == d * d
            qualities += jd(mean) + "\t" + jd(math.sqrt(div(ssd, n))) + "\n"
    files = {".errorprofile": ep, ".indelprofile": jd(ins_all) + "\t" + jd(del_all), ".errorprofile.vcf": vcf,
             ".qualityPerMismatch": qpm, ".indels": indels, ".qualities": qualities}
    return {k: v.encode() for k, v in files.items()}


def infer_files(sam_path, fasta_path, max_read_len, infer_qualities):
    return infer(open(sam_path).read(), read_fasta(fasta_path), max_read_len, infer_qualities)
