"""Host-side mirror of the reference's mapping classes for the hot path.

Same names, argument meaning and error behaviour as
  Mapping.executeMapping(int threads, String reference, String input, String outputPrefix,
                         int mappingQualityFilter, String additionalOptions)   (Mapping.java:40-42)
  PARAsuiteMapping (+ setErrorProfileFilename / setIndelProfileFilename)      (PARAsuiteMapping.java:22-154)
  BWAMapping                                                                    (BWAMapping.java:20-128)
with the three `bwa` child processes replaced by calls into libparasuite_hip.so.  What the Java does
after `bwa samse` -- samtools view -bS / view -q, rm, mv (PARAsuiteMapping.java:102-152), later samtools
sort / index (Mapping.java:85-108) -- is offered as ONE library call, `samToFilteredBam` (SURVEY.md §8f rank 3,
`ps_sam_to_bam`: BAM, MAPQ filter, coordinate sort and .bai without samtools); `<prefix>.sam` is left in place
unless that method is called, and the MAPQ filter also exists on the SAM text.
"""
import os
import time

from . import capi


class ExternalCallErrorException(Exception):
    """mirror of mapping.ExternalCallErrorException: the failing 'command' is carried along"""

    def __init__(self, command):
        super().__init__(command)
        self.command = command

    def getMappingCommand(self):
        return self.command


def _call(what, fn, *args, **kw):
    """Mapping.executeCommand's contract (Mapping.java:151-198): non-zero status => abort with the command; else the call's result"""
    try:
        return fn(*args, **kw)
    except capi.PsError as e:
        raise ExternalCallErrorException("%s: %s" % (what, e))


def _index_unless_present(reference):
    """`bwa index` for a reference whose .bwt is missing (BWAMapping.java:35-45, PARAsuiteMapping.java:45-55)"""
    if not os.path.exists(reference + ".bwt"):
        _call("bwa index " + reference, capi.ps_index, reference)


class Mapping:
    """abstract mirror of mapping.Mapping (Mapping.java:26-206)"""

    def __init__(self):
        self._t0 = None
        self.searchOptions = None

    def setSearchOptions(self, search):
        """the `bwa aln` / `bwa samse` options beyond -n / -X for executeMapping: a capi.SearchOpts, a dict of its fields, or None
        (upstream's defaults).  The other routes (executeMappingToBam, executeMappingWithProfile, Main.map) keep the defaults."""
        self.searchOptions = search

    def executeMapping(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions):
        raise NotImplementedError

    def setTimeStart(self):
        self._t0 = time.time()

    def calculatePassedTime(self):
        return int(time.time() - self._t0)          # whole seconds, as Mapping.java:203-206

    _call = staticmethod(_call)

    def samToFilteredBam(self, outputPrefix, mappingQualityFilter, sortByCoordinateAndIndex=False, threads=8):
        """<prefix>.sam -> <prefix>.bam holding the reads with MAPQ >= filter (PARAsuiteMapping.java:102-152), optionally
        coordinate-sorted with <prefix>.bam.bai (Mapping.sortByCoordinateAndIndex, Mapping.java:85-108); removes the SAM"""
        self._call("samtools view -bS | view -q %d%s" % (mappingQualityFilter, " | sort | index" if sortByCoordinateAndIndex else ""),
                   capi.ps_sam_to_bam, outputPrefix + ".sam", outputPrefix + ".bam", mappingQualityFilter,
                   sortByCoordinateAndIndex, sortByCoordinateAndIndex, threads)
        os.remove(outputPrefix + ".sam")

    def _map_to_bam(self, what, threads, mm, ep, ip, reference, input, outputPrefix, mappingQualityFilter, sortByCoordinateAndIndex):
        """the mapping call and samToFilteredBam fused (`ps_map_to_bam`): <prefix>.bam straight from the alignment records, the 2 GB of
        <prefix>.sam per 10 M reads are never written; BGZF blocks are compressed while later pieces of the input are searched"""
        _index_unless_present(reference)
        self.setTimeStart()
        self._call(what + " | samtools view -bS | view -q %d%s" % (mappingQualityFilter, " | sort | index" if sortByCoordinateAndIndex else ""),
                   capi.ps_map_to_bam, threads, mm, ep, ip, reference, input, outputPrefix + ".bam", mappingQualityFilter,
                   sortByCoordinateAndIndex, sortByCoordinateAndIndex)
        self.seconds = self.calculatePassedTime()

    @staticmethod
    def filter_sam_mapq(sam_in, sam_out, min_mapq):
        """what `samtools view -q Q` keeps (PARAsuiteMapping.java:121-133), on SAM text"""
        with open(sam_in) as fi, open(sam_out, "w") as fo:
            for line in fi:
                if line.startswith("@") or int(line.split("\t", 5)[4]) >= min_mapq:
                    fo.write(line)


class BWAMapping(Mapping):
    """first pass with stock penalties: `bwa aln -t T -n <mm>` + `bwa samse` (BWAMapping.java:51-75)"""

    def executeMapping(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions):
        _index_unless_present(reference)
        self.setTimeStart()
        self._call("bwa aln -t %d -n %s %s %s | bwa samse" % (threads, additionalOptions, reference, input),
                   capi.ps_map, threads, additionalOptions, None, None, reference, input, outputPrefix + ".sam", self.searchOptions)
        self.seconds = self.calculatePassedTime()

    def executeMappingToBam(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions, sortByCoordinateAndIndex=False):
        """executeMapping + samToFilteredBam in one library call (BWAMapping.java:51-128 end to end), no SAM file"""
        self._map_to_bam("bwa aln -t %d -n %s %s %s | bwa samse" % (threads, additionalOptions, reference, input), threads, additionalOptions,
                         None, None, reference, input, outputPrefix, mappingQualityFilter, sortByCoordinateAndIndex)

    def executeMappingWithProfile(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions, maxReadLength):
        """the first pass of a --refine run and the ErrorProfiling step behind it (Main.java:288-334) as ONE call: the profile of
        the alignments with MAPQ >= mappingQualityFilter is counted from memory while the SAM is written (`ps_map_profiled`);
        returns the two file names Main hands to PARAsuiteMapping (<outputPrefix>.bam.errorprofile / .indelprofile)"""
        _index_unless_present(reference)
        self.setTimeStart()
        prefix = outputPrefix + ".bam"                                    # Main.java:335-338: genomicMappingFileName + ".errorprofile"
        self._call("bwa aln -t %d -n %s %s %s | bwa samse | ErrorProfiling" % (threads, additionalOptions, reference, input),
                   capi.ps_map_profiled, threads, additionalOptions, None, None, reference, input, outputPrefix + ".sam",
                   mappingQualityFilter, maxReadLength, prefix)
        self.seconds = self.calculatePassedTime()
        return prefix + ".errorprofile", prefix + ".indelprofile"


class PARAsuiteMapping(Mapping):
    """refine pass with the error profile: `bwa parasuite -t T -X mm -p EP -g IP` + `bwa samse`
    (PARAsuiteMapping.java:63-92)"""

    def __init__(self):
        super().__init__()
        self.errorProfileFilename = None
        self.indelProfileFilename = None

    def setErrorProfileFilename(self, errorProfileFilename):
        self.errorProfileFilename = errorProfileFilename

    def setIndelProfileFilename(self, indelProfileFilename):
        self.indelProfileFilename = indelProfileFilename

    def executeMapping(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions):
        _index_unless_present(reference)
        self.setTimeStart()
        if not self.errorProfileFilename:
            raise ExternalCallErrorException("bwa parasuite: no error profile set (-p)")
        self._call("bwa parasuite -t %d -X %s -p %s -g %s %s %s | bwa samse" %
                   (threads, additionalOptions, self.errorProfileFilename, self.indelProfileFilename, reference, input),
                   capi.ps_map, threads, additionalOptions, self.errorProfileFilename, self.indelProfileFilename,
                   reference, input, outputPrefix + ".sam", self.searchOptions)
        self.seconds = self.calculatePassedTime()

    def executeMappingToBam(self, threads, reference, input, outputPrefix, mappingQualityFilter, additionalOptions, sortByCoordinateAndIndex=False):
        """executeMapping + samToFilteredBam in one library call (PARAsuiteMapping.java:63-152 end to end), no SAM file"""
        if not self.errorProfileFilename:
            raise ExternalCallErrorException("bwa parasuite: no error profile set (-p)")
        self._map_to_bam("bwa parasuite -t %d -X %s -p %s -g %s %s %s | bwa samse" %
                         (threads, additionalOptions, self.errorProfileFilename, self.indelProfileFilename, reference, input), threads, additionalOptions,
                         self.errorProfileFilename, self.indelProfileFilename, reference, input, outputPrefix, mappingQualityFilter, sortByCoordinateAndIndex)


class ErrorProfiling:
    """mirror of utils.errorprofile.ErrorProfiling (ErrorProfiling.java:57-88, 100-631):
    `new ErrorProfiling(mappingFileName, referenceFileName, maxReadLength).inferErrorProfile(isInferQualities, isShowErrorPlot)`
    writes the six files the Java writes, counted on the GPU (`ps_error_profile_full`): <mappingFileName>.errorprofile and
    .indelprofile, which the refine pass reads (Main.java:327-334), and .errorprofile.vcf, .qualityPerMismatch, .indels and
    .qualities (mean and standard deviation of the base quality per read position; empty unless isInferQualities), the files
    of the `error` mode that the PAR-CLIP simulator takes as its indel_file and quality_file.  isShowErrorPlot (a Swing window)
    is ignored.  Returns the paths of the .errorprofile and .indelprofile files."""

    def __init__(self, mappingFileName, referenceFileName, maxReadLength):
        self.mappingFileName = mappingFileName
        self.referenceFileName = referenceFileName
        self.maxReadLength = maxReadLength

    def inferErrorProfile(self, isInferQualities=False, isShowErrorPlot=False):
        _call("ErrorProfiling %s" % self.mappingFileName, capi.ps_error_profile_full, self.mappingFileName, self.referenceFileName,
              self.maxReadLength, None, bool(isInferQualities))
        return self.mappingFileName + ".errorprofile", self.mappingFileName + ".indelprofile"


class PileupClusters:
    """mirror of utils.pileupclusters.PileupClusters (PileupClusters.java:62-673), the `clust` mode (Main.java:601-639):
    `new PileupClusters().calculateReadPileups(alignmentFile, referenceFile, outputFile, snpVcfFile, minReadCoverage)` writes
    <outputFile>, .ccr.fasta, .ccr.tsv and .report, and <alignmentFile>.sitefrequency.tsv and .sitepositions.tsv, counted on
    the GPU (`ps_pileup_clusters`).  snpVcfFile None or "": no known SNPs; the VCF needs no .tbi.  Returns the stats dict."""

    def calculateReadPileups(self, alignmentFile, referenceFile, outputFile, snpVcfFile, minReadCoverage):
        return _call("PileupClusters %s" % alignmentFile, capi.ps_pileup_clusters, alignmentFile, referenceFile, outputFile, snpVcfFile,
                     int(minReadCoverage))


class ExtractWeakMappingReads:
    """mirror of utils.postprocessing.ExtractWeakMappingReads (ExtractWeakMappingReads.java:40-94), step 2 of `map -t`
    (Main.java:363-377): `new ExtractWeakMappingReads().extractReads(mappingFileName, mappingFileNameNew, unalignedReadFileName,
    mapqThreshold)` moves the reads with MAPQ < mapqThreshold into a FASTQ file and writes the BAM without them
    (`ps_extract_weak_reads`, host code).  The caller renames mappingFileNameNew, as Main does.  Returns the stats dict."""

    def extractReads(self, mappingFileName, mappingFileNameNew, unalignedReadFileName, mapqThreshold):
        return _call("ExtractWeakMappingReads %s" % mappingFileName, capi.ps_extract_weak_reads, mappingFileName, mappingFileNameNew,
                     unalignedReadFileName, int(mapqThreshold))


class ExtractNotMappedReads:
    """mirror of utils.postprocessing.ExtractNotMappedReads (ExtractNotMappedReads.java:33-88), the `extractAligned` mode:
    `new ExtractNotMappedReads().extractReads(mappingFileName, alignedReadFileName)` writes "@" + read name for every record of
    the mapping, in file order (`ps_extract_read_names`, host code).  Returns the stats dict."""

    def extractReads(self, mappingFileName, alignedReadFileName):
        return _call("ExtractNotMappedReads %s" % mappingFileName, capi.ps_extract_read_names, mappingFileName, alignedReadFileName)


class CombineGenomeTranscript:
    """mirror of utils.postprocessing.CombineGenomeTranscript (CombineGenomeTranscript.java:36-666), step 5 of `map -t` and the
    `comb` mode (Main.java:400-404, 438-488): `new CombineGenomeTranscript().combine(genomeMappingFileName,
    transcriptMappingFileName, combinedFileName)` appends the transcript hits, lifted to genome coordinates on the GPU, to the
    genomic records (`ps_combine_genome_transcript`).  htsjdk's writer sorts the result by coordinate, so this does too; the
    index is left to Mapping.sortByCoordinateAndIndex's mirror (`capi.ps_bam_index`).  Returns the stats dict."""

    def combine(self, genomeMappingFileName, transcriptMappingFileName, combinedFileName):
        return _call("CombineGenomeTranscript %s %s" % (genomeMappingFileName, transcriptMappingFileName), capi.ps_combine_genome_transcript,
                     genomeMappingFileName, transcriptMappingFileName, combinedFileName, True, False)


class ValidateBenchmarkStatisticsPARCLIP:
    """mirror of utils.benchmarking.ValidateBenchmarkStatisticsPARCLIP (ValidateBenchmarkStatisticsPARCLIP.java:43-242), the
    `benchmark` mode (Main.java:489-521): `new ValidateBenchmarkStatisticsPARCLIP().calculateBenchmarkStatistics(mappingFileName,
    outStatistics, readsFile, onlyBoundClusters)` scores a mapping of simulated PAR-CLIP reads against the truth in the read names
    and writes the six lines of outStatistics, counted on the GPU (`ps_benchmark_reads`).  onlyBoundClusters is accepted and
    ignored, as the Java ignores it (:120-125).  Returns the stats dict."""

    def calculateBenchmarkStatistics(self, mappingFileName, outStatistics, readsFile, onlyBoundClusters=False):
        return _call("ValidateBenchmarkStatisticsPARCLIP %s %s" % (mappingFileName, readsFile), capi.ps_benchmark_reads, mappingFileName,
                     outStatistics, readsFile)


class Main:
    """mirror of main.Main's `map` mode (Main.java:249-420) for the BWA and PARA-suite mappers, as ONE library call
    (`ps_map_route`): `-q readFileName -r referenceFileName -o outputPrefix [-t transcriptFileName] [-p threads] [-l maxReadLength]
    [--gm ..] [--tm ..] [--refine] [--bwa-mm ..] [--parasuite-mm ..] [--parasuite-ep profileFileName --parasuite-indel
    indelFileName]`.  Leaves the files Main.java names and returns what the Java calls mappingFileName: <prefix>.combined.bam with
    a transcript file, else the last genomic mapping.  `stats` holds the call's ps_route_stats afterwards."""

    stats = None

    @staticmethod
    def mappingFileName(outputPrefix, transcriptFileName=None, refine=False):
        if transcriptFileName:
            return outputPrefix + ".combined.bam"
        return outputPrefix + (".PARAsuite-genomic.bam" if refine else ".BWA-genomic.bam")

    def map(self, readFileName, referenceFileName, outputPrefix, transcriptFileName=None, threads=1, maxReadLength=101,
            mappingQualityFilterGenomic=10, mappingQualityFilterTranscript=1, refine=False, bwaMismatches="2",
            parasuiteMismatches="-1", profileFileName=None, indelFileName=None, keepUnaligned=False, referenceRefineFileName=None,
            search=None):
        """keepUnaligned (--unaligned), referenceRefineFileName (--ref-refine) and search (a capi.SearchOpts or a dict of its
        fields, for every pass) go through `ps_map_route_opts`; without them the call is `ps_map_route`"""
        kw = dict(transcripts_fa=transcriptFileName, threads=threads, refine=refine, max_read_len=maxReadLength,
                  mapq_genomic=mappingQualityFilterGenomic, mapq_transcript=mappingQualityFilterTranscript,
                  bwa_mm=bwaMismatches, parasuite_mm=parasuiteMismatches, error_profile=profileFileName, indel_profile=indelFileName)
        route = capi.ps_map_route
        if keepUnaligned or referenceRefineFileName or search is not None:
            route = capi.ps_map_route_opts
            kw.update(keep_unaligned=keepUnaligned, ref_refine=referenceRefineFileName, search=search)
        self.stats = _call("map -q %s -r %s -o %s" % (readFileName, referenceFileName, outputPrefix), route, readFileName, referenceFileName,
                           outputPrefix, **kw)
        return self.mappingFileName(outputPrefix, transcriptFileName, refine)
