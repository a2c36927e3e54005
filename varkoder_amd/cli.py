"""`python -m varkoder_amd image ...`: steps D+E of `varKoder image` on the GPU
(`python -m varkoder_amd convert ...`: `varKoder convert`, see convert.convert_folder).

Same flags as the reference's `image` sub-command (varKoder/cli.py:69-166).  By default the input is the
intermediate folder of a reference run with `-X/--no-image -i INT` (clean + split only, cli.py:155-160), or its
`split_fastqs/` folder: every file `<sample>@<bp>K.fq[.gz]` becomes `<outdir>/<sample>@<bp>K+<mapping>+k<k>.png`
with the reference's metadata.  `--from-clean` enters at step C (cleaned, unsplit reads: the subsample ladder is
drawn on the GPU).  `--from-raw` enters at step B like the reference's own `varKoder image <folder of raw reads>`:
the input is a folder `<taxon>/<sample>/<reads>.fq[.gz]` or a CSV `labels,sample,files`, the reads are cleaned on
the GPU (rules: INTEGRATION.md, "Step B"; -a/-D/-r/-T take effect, -M sets the read budget) and go on to the ladder
without leaving the device; with `-i INT` the cleaned reads and their base-content report are also written to
`INT/clean_reads/` (and reused there by a later run unless -x).  With `--write-splits` (and `-i INT`) both entries also
write every subsample's reads to `INT/split_fastqs/`, the folder the default entry takes (rules: INTEGRATION.md,
"Step C"), and `-X` then stops after these intermediates.  `stats.csv` (and `labels.csv` with -t) are written
like process_stats does (commands/image.py:1144-1185).  With torchrun, ranks shard the files (samples).

`python -m varkoder_amd query ...`: `varKoder query` (run_query); with `--from-raw` from raw reads, cleaned on the GPU
like `image --from-raw`.

`python -m varkoder_amd train ...`: `varKoder train` (train.run_train) with the reference's flags; it writes the model and
label files `query` takes.
"""
import argparse
import math
import os
import shutil
import sys
from collections import OrderedDict, defaultdict
from pathlib import Path

from . import __version__
from .config import (DEFAULT_KMER_MAPPING, DEFAULT_KMER_SIZE, KMER_MAX, KMER_MIN, LABELS_SEP, MAPPING_CHOICES,
                     QUAL_THRESH, SAMPLE_BP_SEP)
from .image import eprint


def add_adapter_flags(p):
    """The adapters-by-sequence flags of `image` and `query` (parse_args refuses them without --from-raw or with -a)."""
    # (SUPPRESS: a namespace without these flags is the one from before they existed; read them with getattr)
    p.add_argument("--detect-adapters", action="store_true", default=argparse.SUPPRESS,
                   help="with --from-raw: also detect each read group's adapter from its first reads and trim it by "
                        "sequence (fastp's adapter detection, as INTEGRATION.md restates it)")
    p.add_argument("--adapter-sequence", default=argparse.SUPPRESS, metavar="SEQ",
                   help="with --from-raw: trim R1 and single reads by this adapter (4-64 bases of ACGT)")
    p.add_argument("--adapter-sequence-r2", default=argparse.SUPPRESS, metavar="SEQ",
                   help="with --from-raw: trim R2 by this adapter (default: --adapter-sequence)")


def setup_parser():
    main = argparse.ArgumentParser(prog="varkoder_amd", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                   description="MI355X-native k-mer counting and varKode/rfCGR imaging")
    sub = main.add_subparsers(required=True, dest="command")
    p = sub.add_parser("image", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="count k-mers and write images for already cleaned + split reads")
    p.add_argument("input", help="intermediate folder of a `varKoder image -X -i` run (or its split_fastqs/)")
    p.add_argument("-R", "--seed", type=int, help="random seed (accepted for parity; nothing here is random)")
    p.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    p.add_argument("-v", "--verbose", action="store_true", default=False)
    p.add_argument("-vv", "--version", action="version", version=f"%(prog)s {__version__}")
    p.add_argument("-k", "--kmer-size", type=int, default=DEFAULT_KMER_SIZE, help="size of kmers to count (5-9)")
    p.add_argument("-p", "--kmer-mapping", type=str, default=DEFAULT_KMER_MAPPING, choices=MAPPING_CHOICES)
    p.add_argument("-n", "--n-threads", type=int, default=1, help="host threads for file reading / PNG writing")
    p.add_argument("-c", "--cpus-per-thread", type=int, default=1, help="accepted for parity, unused")
    p.add_argument("-o", "--outdir", default="images", help="path to folder where to write final images.")
    p.add_argument("-f", "--stats-file", default="stats.csv", help="path to file where sample statistics will be saved.")
    p.add_argument("-i", "--int-folder", help="with --from-raw: folder for the cleaned reads (clean_reads/); "
                                              "otherwise accepted for parity (the input IS the intermediate folder)")
    p.add_argument("-m", "--min-bp", type=str, default="500K",
                   help="with --from-raw / --from-clean: smallest subsample; otherwise applied upstream by the split step")
    p.add_argument("-M", "--max-bp", default="200M",
                   help="with --from-raw / --from-clean: largest subsample (and, --from-raw, 5x of it the read budget); "
                        "otherwise applied upstream by the split step")
    p.add_argument("-t", "--label-table", action="store_true", help="also write labels.csv")
    p.add_argument("-a", "--no-adapter", action="store_true", help="with --from-raw: no adapter trimming; otherwise accepted for parity")
    p.add_argument("-D", "--no-deduplicate", action="store_true", help="with --from-raw: no deduplication; otherwise accepted for parity")
    p.add_argument("-r", "--no-merge", action="store_true", help="with --from-raw: no merging of read pairs; otherwise accepted for parity")
    p.add_argument("-X", "--no-image", action="store_true",
                   help="with --write-splits: stop after the intermediate files (no counting, no images); otherwise "
                        "nothing to do here without images")
    p.add_argument("-T", "--trim-bp", default="10,10",
                   help="with --from-raw: bases trimmed from the front and the tail of every read; otherwise accepted for parity")
    p.add_argument("--labels-csv", help="optional CSV `sample,labels` (labels separated by ';')")
    entry = p.add_mutually_exclusive_group()
    entry.add_argument("--from-clean", action="store_true",
                       help="input holds cleaned but UNSPLIT reads (`<int>/clean_reads/<sample>.fq.gz`): draw the "
                            "1-2-5 ladder of subsamples between --min-bp and --max-bp on the GPU (stands in for "
                            "reformat.sh; statistically equivalent, not the same random reads)")
    entry.add_argument("--from-raw", action="store_true",
                       help="input holds RAW reads (`<taxon>/<sample>/*.fq[.gz]` or a CSV labels,sample,files): clean them "
                            "on the GPU (step B, the reference's fastp pass) and go on with the ladder")
    entry.add_argument("--from-fasta", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                       help="input is a folder of FASTA files (`<sample>.fa|.fasta|.fna[.gz]`: assemblies, contigs, "
                            "organelle genomes): each is counted whole on the GPU and becomes one image "
                            "`<sample>@<bp>K+<mapping>+k<k>.png`, bp = its bases (rule: INTEGRATION.md, \"--from-fasta\")")
    entry.add_argument("--from-bam", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                       help="input is a folder of BAM files (`<sample>.bam`, unaligned or aligned): the records become "
                            "FASTQ text on the GPU and the run goes on as --from-raw does, with its flags (rule: "
                            "INTEGRATION.md, \"--from-bam: the rule\")")
    add_bam_flags(p)
    p.add_argument("--fragments", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-fasta: image every sample as the 1-2-5 ladder of subsamples between --min-bp and "
                        "--max-bp, like --from-clean does for reads, each step drawn from fragments of --fragment-length "
                        "bases of the assembly (rule: INTEGRATION.md, \"--from-fasta --fragments\")")
    p.add_argument("--fragment-length", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --from-fasta --fragments: bases of a fragment, 16 to 1000000 (150 when absent)")
    add_record_flags(p)
    p.add_argument("--write-splits", action="store_true", default=argparse.SUPPRESS,   # (absent = off, as the adapter flags)
                   help="with --from-raw / --from-clean and -i INT: also write every subsample's reads to "
                        "`INT/split_fastqs/<sample>@<bp>K.fq.gz`, the files the default entry takes (kept unless -x "
                        "when a sample's files are all there)")
    p.add_argument("--gpu-gzip", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="compress the .fq.gz files that this run writes (`INT/clean_reads/` with --from-raw and -i INT, "
                        "`INT/split_fastqs/` with --write-splits) on the GPU, as BGZF, and copy back the compressed bytes "
                        "only; without it the host's gzip (level 1) compresses them")
    p.add_argument("--gpu-png", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="encode the image files on the GPU (filter 0, the project's own DEFLATE blocks) and leave the host "
                        "only the writing; pixels and text chunks are the same as without it, the files' bytes are not. "
                        "Not with -X")
    add_adapter_flags(p)
    add_screen_flags(p)
    add_qc_flag(p)
    add_spectrum_flags(p)
    q = sub.add_parser("query", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="Query raw reads, cleaned reads or images against a trained network (cli.py:327-446).")
    q.add_argument("input", help="folder with cleaned reads (`<sample>.fq[.gz]`, e.g. <int>/clean_reads); with --from-raw, "
                                 "with raw reads (one file per sample, or one sub-folder per sample); with --images, "
                                 "with varKode / rfCGR png files")
    q.add_argument("outdir", help="path to the folder where results will be saved.")
    q.add_argument("-R", "--seed", type=int, help="random seed.")
    q.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    q.add_argument("-v", "--verbose", action="store_true", default=False)
    q.add_argument("-l", "--model", required=True,
                   help="local TorchScript archive or pickled torch module (fastai / hub models are not loadable here)")
    q.add_argument("--vocab", required=True, help="text file, one label per output unit of the model")
    q.add_argument("--single-label", action="store_true", help="softmax + best label instead of sigmoid >= threshold")
    q.add_argument("--input-size", type=int, default=224, help="side of the model's input (squish, BOX filter)")
    q.add_argument("--half", action="store_true", help="run the model under fp16 autocast")
    q.add_argument("-1", "--no-pairs", action="store_true",
                   help="accepted for parity and inert: the reference's input listing never reads it either")
    q.add_argument("-I", "--images", action="store_true", help="input folder contains processed images instead of reads.")
    q.add_argument("-k", "--kmer-size", type=int, default=DEFAULT_KMER_SIZE, help="size of kmers to count (5-9)")
    q.add_argument("-p", "--kmer-mapping", type=str, default=DEFAULT_KMER_MAPPING, choices=MAPPING_CHOICES)
    q.add_argument("-n", "--n-threads", type=int, default=1, help="host threads for file reading / PNG writing")
    q.add_argument("-c", "--cpus-per-thread", type=int, default=1, help="accepted for parity, unused")
    q.add_argument("-f", "--stats-file", default="stats.csv", help="path to file where sample statistics will be saved.")
    q.add_argument("-d", "--threshold", type=float, default=0.7, help="confidence threshold to make a prediction.")
    q.add_argument("-i", "--int-folder", help="with --from-raw: folder for the cleaned reads (clean_reads/), reused by a "
                                              "later run unless -x; otherwise accepted for parity")
    q.add_argument("-m", "--keep-images", action="store_true",
                   help="whether barcode images should be saved to a directory named 'query_images'.")
    q.add_argument("-P", "--include-probs", action="store_true",
                   help="whether probabilities for each label should be included in the output.")
    q.add_argument("-a", "--no-adapter", action="store_true", help="with --from-raw: no adapter trimming; otherwise accepted for parity")
    q.add_argument("-r", "--no-merge", action="store_true", help="with --from-raw: no merging of read pairs; otherwise accepted for parity")
    q.add_argument("-D", "--no-deduplicate", action="store_true", help="with --from-raw: no deduplication; otherwise accepted for parity")
    q.add_argument("-T", "--trim-bp", default="10,10",
                   help="with --from-raw: bases trimmed from the front and the tail of every read; otherwise accepted for parity")
    q.add_argument("-M", "--max-bp", default="200M",
                   help="number of post-cleaning basepairs to use for making image (and, --from-raw, 5x of it the read "
                        "budget). Use '0' to use all of the available data.")
    q.add_argument("--from-raw", action="store_true",
                   help="input holds RAW reads, as the reference's `query` takes them: clean them on the GPU (step B, the "
                        "reference's fastp pass), subsample, image and predict without leaving the device")
    q.add_argument("--from-fasta", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="input is a folder of FASTA files (`<sample>.fa|.fasta|.fna[.gz]`), one sample each: counted whole "
                        "on the GPU, imaged and predicted")
    q.add_argument("--from-bam", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="input is a folder of BAM files (`<sample>.bam`), one sample each: converted to reads on the GPU, "
                        "then as --from-raw")
    add_bam_flags(q)
    add_record_flags(q)
    q.add_argument("--gpu-gzip", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-raw and -i INT: compress the cleaned reads on the GPU, as BGZF, and copy back the "
                        "compressed bytes only")
    q.add_argument("--gpu-png", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with -m/--keep-images: encode the kept images on the GPU; pixels and text chunks are the same as "
                        "without it, the files' bytes are not")
    q.add_argument("--gpu-png-read", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with -I/--images: decode the image files on the GPU (8-bit greyscale square files up to 512 a side; "
                        "any other file, and any the decoder refuses, is decoded by PIL as without the flag); the "
                        "predictions are the same. Measured: 4,000 files of 128 x 128 in 80 ms against 403 ms, 400 of "
                        "512 x 512 in 36 ms against 313 ms (profiles/ab/unpng_time.txt)")
    add_adapter_flags(q)
    add_screen_flags(q)
    add_qc_flag(q)
    add_spectrum_flags(q)
    q.add_argument("-b", "--max-batch-size", type=int, default=64, help="maximum batch size for predictions.")
    c = sub.add_parser("convert", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="Convert images between different kmer mappings.")          # cli.py:447-482
    c.add_argument("-R", "--seed", type=int, help="accepted for parity")
    c.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    c.add_argument("-v", "--verbose", action="store_true", default=False)
    c.add_argument("-n", "--n-threads", type=int, default=1, help="host threads for reading / writing PNG files")
    c.add_argument("-k", "--kmer-size", type=int, default=DEFAULT_KMER_SIZE, choices=[5, 6, 7, 8, 9],
                   help="size of kmers used to produce original images (as in the reference, this value "
                        "takes priority over the file names)")
    c.add_argument("-p", "--input-mapping", choices=MAPPING_CHOICES,
                   help="kmer mapping of input images. Will be inferred from file names if omitted.")
    c.add_argument("-r", "--sum-reverse-complements", action="store_true",
                   help="When converting from CGR to varKode, add together counts from canonical kmers and "
                        "their reverse complements.")
    c.add_argument("output_mapping", choices=MAPPING_CHOICES, help="kmer mapping of output images.")
    c.add_argument("input", help="path to folder with png images files to be converted.")
    c.add_argument("outdir", help="path to the folder where results will be saved.")
    t = sub.add_parser("train", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="Train a neural network on images (cli.py:168-323); batches are built on the GPU.")
    t.add_argument("input", help="path to the folder with input images.")
    t.add_argument("outdir", help="path to the folder where trained model will be stored.")
    t.add_argument("-R", "--seed", type=int, help="random seed (split, weights, order and augmentation).")
    t.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    t.add_argument("-v", "--verbose", action="store_true", default=False)
    t.add_argument("-n", "--num-workers", type=int, default=0, help="accepted for parity and inert: there are no loader workers")
    t.add_argument("-t", "--label-table-path", help="csv table `sample,labels`; by default labels come from the image metadata.")
    t.add_argument("-S", "--single-label", action="store_true",
                   help="single-label model; several labels of a sample are concatenated to one.")
    t.add_argument("-d", "--threshold", type=float, default=0.7,
                   help="threshold of the validation precision and recall. Ignored with --single-label")
    t.add_argument("-V", "--validation-set", help="comma-separated sample IDs of the validation set, or a file with such a list.")
    t.add_argument("-f", "--validation-set-fraction", type=float, default=0.2,
                   help="fraction of samples held out per label combination. Ignored with --validation-set.")
    t.add_argument("-c", "--architecture", default="hf-hub:brunoasm/vit_large_patch32_224.NCBI_SRA",
                   help="arias2022, fiannaca2018, vit_l32 or pkg.module:factory (the reference's default and timm names "
                        "are refused: timm is not assumed here)")
    t.add_argument("-m", "--pretrained-model", help="model file (as `query -l` loads it) whose matching weights start the training.")
    t.add_argument("-b", "--max-batch-size", type=int, default=64, help="maximum batch size.")
    t.add_argument("-B", "--min-batch-size", type=int, default=1, help="minimum batch size.")
    t.add_argument("-C", "--cpu", action="store_true", default=False, help="refused: there is no CPU path")
    t.add_argument("-r", "--base-learning-rate", type=float, default=5e-3, help="base learning rate.")
    t.add_argument("-e", "--epochs", type=int, default=30, help="number of epochs to train.")
    t.add_argument("-z", "--freeze-epochs", type=int, default=0, help="epochs that train the last linear layer only, first.")
    t.add_argument("-w", "--random-weights", action="store_true",
                   help="accepted for parity and inert: weights are random unless -m is given")
    t.add_argument("-i", "--negative_downweighting", type=float, default=4,
                   help="gamma(negative) of the asymmetric loss (arXiv:2009.14119). Ignored with --single-label.")
    t.add_argument("-X", "--mix-augmentation", choices=["CutMix", "MixUp", "None"], default="MixUp")
    t.add_argument("-s", "--label-smoothing", action="store_true", default=False,
                   help="label smoothing 0.1. Only with --single-label and a mix augmentation.")
    t.add_argument("-p", "--p-lighting", type=float, default=0.75, help="probability of a lighting transform; 0 for none.")
    t.add_argument("-l", "--max-lighting", type=float, default=0.25, help="maximum scale of the lighting transform.")
    t.add_argument("-g", "--no-logging", action="store_true", default=False, help="no per-epoch lines on stderr.")
    t.add_argument("-M", "--no-metrics", action="store_true", default=False, help="skip validation loss and metrics.")
    t.add_argument("--input-size", type=int, default=224,
                   help="side of the input of vit_l32 and of a pkg.module:factory model (squish, BOX filter); arias2022 and "
                        "fiannaca2018 take the images at their own size")
    t.add_argument("--gpu-png-read", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="decode the image files on the GPU (8-bit greyscale square files up to 512 a side; any other "
                        "file, and any the decoder refuses, is decoded by PIL as without the flag); the training set is "
                        "the same. Measured: 4,000 files of 128 x 128 in 80 ms against 403 ms, 400 of 512 x 512 in 36 ms "
                        "against 313 ms (profiles/ab/unpng_time.txt)")
    m = sub.add_parser("compare", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="Nearest neighbours among images by exact squared Euclidean distance, computed on the GPU "
                            "(no model; not in the reference).")
    m.add_argument("input", help="path to the folder with the images to compare (IMAGES).")
    m.add_argument("outdir", help="path to the folder where neighbours.csv and samples.csv will be written (OUT).")
    m.add_argument("--against", metavar="REF_IMAGES",
                   help="folder of reference images: the neighbours of every image of IMAGES are looked for among these, "
                        "without exclusions. By default IMAGES is compared with itself.")
    m.add_argument("-N", "--neighbours", type=int, default=10, help="neighbours per image, 1 to 64.")
    m.add_argument("--same-sample", action="store_true", default=False,
                   help="let the other images of an image's own sample (its other bp steps) be its neighbours: only the "
                        "image itself is excluded. Not with --against.")
    m.add_argument("--matrix", action="store_true", default=False,
                   help="also write every distance: distances.npy (uint64) with distances_rows.txt and distances_cols.txt; "
                        "refused above 4 GiB.")
    m.add_argument("-t", "--label-table", help="csv table `sample,labels`; by default labels come from the image metadata.")
    m.add_argument("--gpu-png-read", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="decode the image files on the GPU, as `train --gpu-png-read` does; the images are the same.")
    m.add_argument("-n", "--n-threads", type=int, default=1, help="accepted for parity and inert: the files are read in turn")
    m.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    m.add_argument("-v", "--verbose", action="store_true", default=False)
    d = sub.add_parser("distance", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       help="Genomic distances between samples from the sketches that `--kmer-spectrum DIR "
                            "--spectrum-sketch S` (reads) and `--from-fasta --genome-spectrum DIR --spectrum-sketch S` "
                            "(assemblies) wrote, every pair compared on the GPU (not in the reference; rule and "
                            "limits: INTEGRATION.md, \"`--spectrum-sketch` and `distance`: the rule\").")
    d.add_argument("input", help="path to the folder with the samples' .spectrum.json and .sketch.npy files (SPECTRA).")
    d.add_argument("outdir", help="path to the folder where distances.csv will be written (OUT).")
    d.add_argument("--against", metavar="REF_SPECTRA",
                   help="folder of reference samples: the neighbours of every sample of SPECTRA are looked for among these. "
                        "By default SPECTRA is compared with itself, a sample never with itself.")
    d.add_argument("-N", "--neighbours", type=int, default=10, help="neighbours per sample, 1 at least.")
    d.add_argument("--matrix", action="store_true", default=False,
                   help="also write every pair: shared.npy, seen.npy (uint32), corrected_distance.npy (float64, NaN where "
                        "there is none) with distances_rows.txt and distances_cols.txt.")
    d.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    t = sub.add_parser("tree", formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                       usage="%(prog)s SPECTRA OUT [--distance corrected|mash] [--jukes-cantor] [--replicates R] [--seed N] "
                             "[--no-negative-branches] [-x]\n       %(prog)s --matrix-from DIR OUT [--no-negative-branches] [-x]",
                       help="A neighbour-joining tree of the sketched samples of a folder (as `distance` reads it), or of "
                            "a matrix that `distance --matrix` or `compare --matrix` wrote; every matrix is joined on the "
                            "GPU (not in the reference; rule and limits: INTEGRATION.md, \"`tree`: the rule\"). Writes "
                            "tree.nwk (Newick, unrooted) and tree.json (the join record and every split's support).")
    t.add_argument("paths", nargs="+", metavar="PATH",
                   help="SPECTRA OUT: the folder with the samples' .spectrum.json and .sketch.npy files, and the folder "
                        "where tree.nwk and tree.json will be written. With --matrix-from: OUT alone.")
    t.add_argument("--matrix-from", metavar="DIR",
                   help="join the square matrix of DIR instead: corrected_distance.npy (`distance --matrix`) or "
                        "distances.npy (`compare --matrix`, uint64, refused above 2^53) with distances_rows.txt and "
                        "distances_cols.txt, which must agree. No replicates in this mode.")
    t.add_argument("--distance", choices=("corrected", "mash"), default="corrected",
                   help="the distance of every pair: the depth-corrected one or the Mash distance (`distance` writes "
                        "both). A pair without one (nothing seen, a sample without estimates) is refused by name.")
    t.add_argument("--jukes-cantor", action="store_true", default=False,
                   help="transform every distance D to -0.75 ln(1 - 4D/3), substitutions per site under Jukes and "
                        "Cantor's model; a D of 0.75 or more is refused by name.")
    t.add_argument("--replicates", type=int, default=0, metavar="R",
                   help="support values from R delete-half jackknife replicates: each keeps 32 of the 64 blocks the "
                        "sketch values fall into (by their low 6 bits) and builds its tree from the kept blocks' counts; "
                        "an inner node is labelled with the percentage of replicate trees that hold its split. This "
                        "measures the sampling variance of the SKETCH, not variance among reads or loci: a split can be "
                        "well supported and wrong, and support rises with the sketch size. A replicate with an undefined "
                        "distance is dropped and counted; more than half dropped is refused. At most 4095.")
    t.add_argument("--seed", type=int, default=1, metavar="N",
                   help="seed of the replicates' block choice (a generator written out in tree.py: the same blocks with "
                        "every NumPy).")
    t.add_argument("--no-negative-branches", action="store_true", default=False,
                   help="in tree.nwk set a negative length of a joined pair to 0 and give the difference to its sibling "
                        "(Kuhner and Felsenstein 1994: the path through the pair keeps its length); tree.json keeps the "
                        "lengths as computed.")
    t.add_argument("-x", "--overwrite", action="store_true", help="overwrite existing results.")
    return main


MIN_RECORD_LENGTH_DEFAULT = 1000
WINDOW_LENGTH_DEFAULT = 10000


def add_bam_flags(p):
    p.add_argument("--bam-pairs", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-bam: a file's first mates (flag & 0xC1 == 0x41), second mates (0x81) and other reads "
                        "are the R1, R2 and unpaired files of its sample; mates must appear in the same order (unaligned "
                        "or collated BAMs): a file sorted by coordinate is refused")
    p.add_argument("--bam-read-groups", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-bam: every read group of a file (the ID: of an @RG line of its header) is a sample "
                        "`<file>__<id>` of the reads whose RG:Z tag names it, split on the GPU; reads of no listed group are "
                        "passed over and counted on stderr (INTEGRATION.md, \"--from-bam --bam-read-groups: the rule\")")
    p.add_argument("--bam-exclude", type=lambda t: int(t, 0), default=argparse.SUPPRESS, metavar="INT",
                   help="with --from-bam: records with any of these flag bits are passed over (0x900 when absent: "
                        "secondary and supplementary, as `samtools fastq`; 0xF00 also drops QC-fail and duplicates)")


def bam_options(args):
    """raw_to_images' / raw_to_query's `bam` of `--from-bam`, None without the flag."""
    if not getattr(args, "from_bam", False):
        return None
    from .bam import EXCLUDE_DEFAULT
    return dict(pairs=getattr(args, "bam_pairs", False), exclude=getattr(args, "bam_exclude", EXCLUDE_DEFAULT),
                groups={} if getattr(args, "bam_read_groups", False) else None)   # ({sample: group}: filled by RawPlan)


SCREEN_K_DEFAULT, SCREEN_K_MIN, SCREEN_K_MAX = 31, 16, 31


def add_screen_flags(p):
    which = p.add_mutually_exclusive_group()
    which.add_argument("--exclude-fasta", default=argparse.SUPPRESS, metavar="FILE",   # (absent = no screen)
                       help="where cleaned reads lie on the GPU in front of the subsampling (--from-raw, --from-bam, "
                            "--from-clean; query's cleaned reads): drop every read that shares a k-mer with this reference "
                            "FASTA (.gz or not, any number of records: PhiX, a host, an organelle) before the subsampling "
                            "(rule: INTEGRATION.md, \"--exclude-fasta / --keep-fasta: the rule\")")
    which.add_argument("--keep-fasta", default=argparse.SUPPRESS, metavar="FILE",
                       help="the converse of --exclude-fasta: keep only the reads that share a k-mer with this reference")
    p.add_argument("--screen-k", type=int, default=argparse.SUPPRESS, metavar="K",
                   help=f"with --exclude-fasta / --keep-fasta: the k-mer size of the screen, {SCREEN_K_MIN} to {SCREEN_K_MAX} "
                        f"({SCREEN_K_DEFAULT} when absent)")
    p.add_argument("--screen-min-hits", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --exclude-fasta / --keep-fasta: a read matches when at least N of its k-mer positions are in "
                        "the reference (1 when absent)")


def add_qc_flag(p):
    p.add_argument("--qc-report", default=argparse.SUPPRESS, metavar="DIR",   # (absent = no report)
                   help="write DIR/<sample>.qc.json: reads, bases, Q20/Q30 rates, GC content, read lengths and per-cycle "
                        "quality and base-content curves of the reads before and after cleaning, counted on the GPU where "
                        "their text lies, and add their columns to stats.csv; where the run starts from cleaned reads "
                        "the report has the `after` sections only (rule: INTEGRATION.md, \"--qc-report: the rule\")")


SPECTRUM_K_DEFAULT, SPECTRUM_K_MIN, SPECTRUM_K_MAX = 21, 16, 31
SKETCH_MIN, SKETCH_MAX = 64, 1 << 20


def add_spectrum_flags(p):
    p.add_argument("--kmer-spectrum", default=argparse.SUPPRESS, metavar="DIR",   # (absent = nothing is counted)
                   help="write DIR/<sample>.spectrum.json: the k-mer spectrum of the cleaned reads (behind the screen, once "
                        "per sample), counted on the GPU where their text lies, with estimates of k-mer and base coverage, "
                        "the genome's distinct k-mers, the error rate and the share of high-copy k-mers, and add their "
                        "columns to stats.csv (--from-raw, --from-bam, --from-clean; query's cleaned reads; rule and limits: "
                        "INTEGRATION.md, \"`--kmer-spectrum`: the rule\")")
    p.add_argument("--genome-spectrum", default=argparse.SUPPRESS, metavar="DIR",   # (absent = nothing is counted)
                   help="with --from-fasta (whole files): write DIR/<sample>.spectrum.json, the k-mer spectrum of the "
                        "assembly counted on the GPU from the FASTA text the image is counted from -- distinct k-mers, "
                        "copy numbers -- with \"source\": \"assembly\"; with --spectrum-sketch also the sketch that "
                        "`distance --against DIR` compares skims with (not in the reference; rule: INTEGRATION.md, "
                        "\"`--genome-spectrum`: the rule\")")
    p.add_argument("--spectrum-k", type=int, default=argparse.SUPPRESS, metavar="K",
                   help=f"with --kmer-spectrum or --genome-spectrum: the k-mer size, {SPECTRUM_K_MIN} to {SPECTRUM_K_MAX} ({SPECTRUM_K_DEFAULT} when absent)")
    p.add_argument("--spectrum-every", type=int, default=argparse.SUPPRESS, metavar="M",
                   help="with --kmer-spectrum or --genome-spectrum: count the k-mers whose hash is a multiple of M, a 1/M sample of the spectrum "
                        "in a table M times smaller (1 when absent: every k-mer, exact)")
    p.add_argument("--spectrum-sketch", type=int, default=argparse.SUPPRESS, metavar="S",
                   help=f"with --kmer-spectrum or --genome-spectrum: also write DIR/<sample>.sketch.npy, the S ({SKETCH_MIN} to {SKETCH_MAX}) smallest "
                        "hashes of the sample's distinct k-mers, taken on the GPU from the table the spectrum was counted "
                        "in, and a \"sketch\" object in its .spectrum.json: what `distance` compares")
    p.add_argument("--spectrum-sketch-min-count", type=int, default=argparse.SUPPRESS, metavar="M",
                   help="with --spectrum-sketch: sketch the k-mers seen M times and more (1 when absent; 2 leaves most "
                        "error k-mers out of a deep sample)")
    p.add_argument("--depth-filter", default=argparse.SUPPRESS, metavar="LO:HI",
                   help="with --kmer-spectrum: keep the reads whose median k-mer depth in their own sample's spectrum lies in "
                        "LO..HI, decided on the GPU against the table the spectrum was counted in; the files, the QC's after "
                        "section and the images see what is kept.  Either end may be empty; an end is a multiplicity (:4 "
                        "images the low-copy, nuclear reads of a skim, 20: the organelle and repeat reads) or a multiple of "
                        "the sample's estimated k-mer coverage (3x:).  The sample's .spectrum.json gains a \"depth_filter\" "
                        "object with the histogram of the reads' median depths (rule: INTEGRATION.md, \"`--depth-filter`: "
                        "the rule\")")


def genome_spectrum_options(args):
    """pipeline.GenomeSpectrum of `--genome-spectrum`, None without it."""
    if not hasattr(args, "genome_spectrum"):
        return None
    from .pipeline import GenomeSpectrum
    return GenomeSpectrum(Path(args.genome_spectrum), getattr(args, "spectrum_k", SPECTRUM_K_DEFAULT),
                          getattr(args, "spectrum_every", 1), getattr(args, "spectrum_sketch", None))


def spectrum_options(args):
    """pipeline.Spectrum of `--kmer-spectrum`, None without it."""
    if not hasattr(args, "kmer_spectrum"):
        return None
    from .pipeline import Spectrum
    return Spectrum(Path(args.kmer_spectrum), getattr(args, "spectrum_k", SPECTRUM_K_DEFAULT), getattr(args, "spectrum_every", 1),
                    getattr(args, "spectrum_sketch", None), getattr(args, "spectrum_sketch_min_count", 1),
                    getattr(args, "depth_band", None))


def qc_options(args):
    """The folder of `--qc-report`, None without it."""
    return Path(args.qc_report) if hasattr(args, "qc_report") else None


def screen_options(args):
    """pipeline.Screen of `--exclude-fasta` / `--keep-fasta`, None without either."""
    keep = hasattr(args, "keep_fasta")
    if not keep and not hasattr(args, "exclude_fasta"):
        return None
    from .pipeline import Screen
    return Screen(Path(args.keep_fasta if keep else args.exclude_fasta), getattr(args, "screen_k", SCREEN_K_DEFAULT),
                  getattr(args, "screen_min_hits", 1), keep)


def add_record_flags(p):
    p.add_argument("--per-record", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-fasta: every RECORD of a FASTA file is a sample of its own, `<file sample>__<id>`, id "
                        "= its header up to the first blank (a reference collection in one multi-FASTA; the contigs of "
                        "an assembly, each on its own; rule: INTEGRATION.md, \"--from-fasta --per-record\")")
    p.add_argument("--min-record-length", type=int, default=argparse.SUPPRESS, metavar="N",
                   help="with --from-fasta --per-record: records of fewer than N bases are passed over, N >= k "
                        f"({MIN_RECORD_LENGTH_DEFAULT} when absent)")
    p.add_argument("--windows", action="store_true", default=argparse.SUPPRESS,   # (absent = off)
                   help="with --from-fasta: every WINDOW of --window-length bases of a record, one every --window-step "
                        "bases, is a sample of its own, `<file sample>__<id>__<start>-<end>` (where along a chromosome a "
                        "foreign stretch lies; fixed-length pieces to train on; no partial windows; rule: "
                        "INTEGRATION.md, \"--from-fasta --windows\")")
    p.add_argument("--window-length", type=int, default=argparse.SUPPRESS, metavar="N",
                   help=f"with --from-fasta --windows: bases of a window, 100 <= N < 2^31 ({WINDOW_LENGTH_DEFAULT} when absent)")
    p.add_argument("--window-step", type=int, default=argparse.SUPPRESS, metavar="S",
                   help="with --from-fasta --windows: bases from one window's start to the next, k <= S <= N, a divisor of N "
                        "with N / S <= 64 (N when absent: windows side by side)")


def window_options(args):
    """fasta_to_images' / fasta_to_query's options of `--windows`, {} without the flag."""
    if not getattr(args, "windows", False):
        return {}
    n = getattr(args, "window_length", WINDOW_LENGTH_DEFAULT)
    return dict(windows=True, window_length=n, window_step=getattr(args, "window_step", n))


ADAPTER_FLAGS = (("detect_adapters", "--detect-adapters"), ("adapter_sequence", "--adapter-sequence"),
                 ("adapter_sequence_r2", "--adapter-sequence-r2"))


FRAGMENT_LENGTH_DEFAULT, FRAGMENT_LENGTH_MIN, FRAGMENT_LENGTH_MAX = 150, 16, 1000000


def parse_args(argv=None):
    """The parsed command line; the adapter flags of `image` and `query` are refused (exit 2) without --from-raw or
    with -a, and their sequences are checked."""
    parser = setup_parser()
    args = parser.parse_args(argv)
    if args.command == "compare":
        if not 1 <= args.neighbours <= 64:
            parser.error("-N/--neighbours: 1 to 64")
        if args.same_sample and args.against:
            parser.error("--same-sample: not with --against (nothing is excluded there)")
        return args
    if args.command == "distance":
        if args.neighbours < 1:
            parser.error("-N/--neighbours: at least 1")
        return args
    if args.command == "tree":
        want = 1 if args.matrix_from else 2
        if len(args.paths) != want:
            parser.error("tree: --matrix-from DIR OUT, or SPECTRA OUT")
        args.input, args.outdir = (args.matrix_from, args.paths[0]) if args.matrix_from else args.paths   # (input: what must exist)
        if args.matrix_from and args.replicates:
            parser.error("--replicates: not with --matrix-from (a matrix carries no sketch to resample)")
        if args.matrix_from and args.jukes_cantor:
            parser.error("--jukes-cantor: not with --matrix-from (the matrix is joined as it is)")
        if not 0 <= args.replicates <= 4095:
            parser.error("--replicates: 0 to 4095")
        if not 0 <= args.seed < 2 ** 64:
            parser.error("--seed: 0 to 2^64 - 1")
        return args
    if args.command == "query" and args.from_raw and args.images:
        parser.error("--from-raw: not with -I/--images")
    from_bam = args.command in ("image", "query") and getattr(args, "from_bam", False)
    if from_bam:   # (image: the entry flags exclude each other in the parser)
        if args.command == "query" and (args.images or args.from_raw or getattr(args, "from_fasta", False)):
            parser.error("--from-bam: not with -I/--images, --from-raw or --from-fasta")
        if hasattr(args, "bam_exclude") and not 0 <= args.bam_exclude <= 0xFFFF:
            parser.error("--bam-exclude: 0 to 0xFFFF")
    if args.command in ("image", "query") and not from_bam:
        for name, flag in (("bam_pairs", "--bam-pairs"), ("bam_exclude", "--bam-exclude"), ("bam_read_groups", "--bam-read-groups")):
            if hasattr(args, name):
                parser.error(f"{flag}: only with --from-bam")
    if getattr(args, "from_fasta", False):   # one image per file, nothing written but images: no ladder, no intermediates
        if args.command == "query" and (args.images or args.from_raw):
            parser.error("--from-fasta: not with -I/--images or --from-raw")
        for name, flag in (("write_splits", "--write-splits"), ("gpu_gzip", "--gpu-gzip")):
            if getattr(args, name, False):
                parser.error(f"--from-fasta: not with {flag}")
    if args.command in ("image", "query"):
        for name, flag in (("per_record", "--per-record"), ("min_record_length", "--min-record-length"), ("windows", "--windows"),
                           ("window_length", "--window-length"), ("window_step", "--window-step")):
            if hasattr(args, name) and not getattr(args, "from_fasta", False):
                parser.error(f"{flag}: only with --from-fasta")
        if hasattr(args, "min_record_length") and not getattr(args, "per_record", False):
            parser.error("--min-record-length: only with --per-record")
        if getattr(args, "per_record", False) and getattr(args, "fragments", False):
            parser.error("--per-record: not with --fragments")
        if hasattr(args, "min_record_length") and args.min_record_length < args.kmer_size:
            parser.error("--min-record-length: at least the k-mer size")
        for name, flag in (("window_length", "--window-length"), ("window_step", "--window-step")):
            if hasattr(args, name) and not getattr(args, "windows", False):
                parser.error(f"{flag}: only with --windows")
        if getattr(args, "windows", False):
            for name, flag in (("fragments", "--fragments"), ("per_record", "--per-record")):
                if getattr(args, name, False):
                    parser.error(f"--windows: not with {flag}")
            from .fasta import window_limits
            opts = window_options(args)
            why = window_limits(opts["window_length"], opts["window_step"], args.kmer_size)
            if why:
                parser.error(f"--window-length, --window-step: {why}")
    if args.command == "image":
        for name, flag in (("fragments", "--fragments"), ("fragment_length", "--fragment-length")):
            if hasattr(args, name) and not getattr(args, "from_fasta", False):
                parser.error(f"{flag}: only with --from-fasta")
        if hasattr(args, "fragment_length") and not FRAGMENT_LENGTH_MIN <= args.fragment_length <= FRAGMENT_LENGTH_MAX:
            parser.error(f"--fragment-length: {FRAGMENT_LENGTH_MIN} to {FRAGMENT_LENGTH_MAX}")
    if args.command == "image" and getattr(args, "write_splits", False):
        if not (args.from_raw or args.from_clean or from_bam):
            parser.error("--write-splits: only with --from-raw or --from-clean (or --from-bam, which runs as --from-raw)")
        if not args.int_folder:
            parser.error("--write-splits: needs -i/--int-folder")
    if args.command in ("image", "query") and getattr(args, "gpu_gzip", False):
        # only where this run writes a .fq.gz: the cleaned reads of --from-raw -i INT, or --write-splits' files
        if not (((args.from_raw or from_bam) and args.int_folder) or getattr(args, "write_splits", False)):
            parser.error("--gpu-gzip: only with --from-raw and -i/--int-folder" +
                         (", or with --write-splits" if args.command == "image" else "") +
                         " (--from-bam counts as --from-raw)")
    if args.command in ("image", "query"):
        which = [flag for name, flag in (("exclude_fasta", "--exclude-fasta"), ("keep_fasta", "--keep-fasta")) if hasattr(args, name)]
        for name, flag in (("screen_k", "--screen-k"), ("screen_min_hits", "--screen-min-hits")):
            if hasattr(args, name) and not which:
                parser.error(f"{flag}: only with --exclude-fasta or --keep-fasta")
        if which:
            # only where cleaned reads lie in HBM in front of the ladder
            if getattr(args, "from_fasta", False):
                parser.error(f"{which[0]}: not with --from-fasta (reads are screened, not assemblies)")
            if args.command == "query" and args.images:
                parser.error(f"{which[0]}: not with -I/--images (no reads)")
            if args.command == "image" and not (args.from_raw or args.from_clean or from_bam):
                parser.error(f"{which[0]}: only with --from-raw, --from-bam or --from-clean (the default entry takes "
                             "subsamples that are drawn already)")
            if hasattr(args, "screen_k") and not SCREEN_K_MIN <= args.screen_k <= SCREEN_K_MAX:
                parser.error(f"--screen-k: {SCREEN_K_MIN} to {SCREEN_K_MAX}")
            if hasattr(args, "screen_min_hits") and args.screen_min_hits < 1:
                parser.error("--screen-min-hits: at least 1")
            ref = getattr(args, "keep_fasta", None) or getattr(args, "exclude_fasta", None)
            if not Path(ref).is_file():
                parser.error(f"{which[0]}: no such file: {ref}")
    if args.command in ("image", "query") and hasattr(args, "qc_report"):
        # only where reads lie in HBM as FASTQ text whole: raw files, BAM files' reads, cleaned reads
        if getattr(args, "from_fasta", False):
            parser.error("--qc-report: not with --from-fasta (assemblies have no qualities)")
        if args.command == "query" and args.images:
            parser.error("--qc-report: not with -I/--images (no reads)")
        if args.command == "image" and not (args.from_raw or args.from_clean or from_bam):
            parser.error("--qc-report: only with --from-raw, --from-bam or --from-clean (the default entry takes "
                         "subsamples that are drawn already)")
    if args.command in ("image", "query"):
        for name, flag in (("spectrum_k", "--spectrum-k"), ("spectrum_every", "--spectrum-every"),
                           ("spectrum_sketch", "--spectrum-sketch"),
                           ("spectrum_sketch_min_count", "--spectrum-sketch-min-count"),
                           ("depth_filter", "--depth-filter")):
            if hasattr(args, name) and not hasattr(args, "kmer_spectrum"):
                if not hasattr(args, "genome_spectrum"):
                    parser.error(f"{flag}: only with --kmer-spectrum" +
                                 (" or --genome-spectrum" if name in ("spectrum_k", "spectrum_every", "spectrum_sketch") else ""))
                if name in ("spectrum_sketch_min_count", "depth_filter"):
                    parser.error(f"{flag}: not with --genome-spectrum (an assembly has no error k-mers to threshold and no depth)")
        if hasattr(args, "genome_spectrum"):
            # only where an assembly's whole text lies in HBM
            if hasattr(args, "kmer_spectrum"):
                parser.error("--genome-spectrum: not with --kmer-spectrum (one counts assemblies, the other reads)")
            if not getattr(args, "from_fasta", False):
                parser.error("--genome-spectrum: only with --from-fasta (reads are counted with --kmer-spectrum)")
            for name, flag in (("fragments", "--fragments"), ("per_record", "--per-record"), ("windows", "--windows")):
                if getattr(args, name, False):
                    parser.error(f"--genome-spectrum: not with {flag} (the spectrum is the whole file's)")
            if hasattr(args, "spectrum_k") and not SPECTRUM_K_MIN <= args.spectrum_k <= SPECTRUM_K_MAX:
                parser.error(f"--spectrum-k: {SPECTRUM_K_MIN} to {SPECTRUM_K_MAX}")
            if hasattr(args, "spectrum_every") and args.spectrum_every < 1:
                parser.error("--spectrum-every: at least 1")
            if hasattr(args, "spectrum_sketch") and not SKETCH_MIN <= args.spectrum_sketch <= SKETCH_MAX:
                parser.error(f"--spectrum-sketch: {SKETCH_MIN} to {SKETCH_MAX}")
        if hasattr(args, "kmer_spectrum"):
            # only where cleaned reads lie in HBM as FASTQ text whole
            if getattr(args, "from_fasta", False):
                parser.error("--kmer-spectrum: not with --from-fasta (the spectrum of reads tells depth; an assembly has none)")
            if args.command == "query" and args.images:
                parser.error("--kmer-spectrum: not with -I/--images (no reads)")
            if args.command == "image" and not (args.from_raw or args.from_clean or from_bam):
                parser.error("--kmer-spectrum: only with --from-raw, --from-bam or --from-clean (the default entry takes "
                             "subsamples that are drawn already)")
            if hasattr(args, "spectrum_k") and not SPECTRUM_K_MIN <= args.spectrum_k <= SPECTRUM_K_MAX:
                parser.error(f"--spectrum-k: {SPECTRUM_K_MIN} to {SPECTRUM_K_MAX}")
            if hasattr(args, "spectrum_every") and args.spectrum_every < 1:
                parser.error("--spectrum-every: at least 1")
            if hasattr(args, "spectrum_sketch") and not SKETCH_MIN <= args.spectrum_sketch <= SKETCH_MAX:
                parser.error(f"--spectrum-sketch: {SKETCH_MIN} to {SKETCH_MAX}")
            if hasattr(args, "spectrum_sketch_min_count"):
                if not hasattr(args, "spectrum_sketch"):
                    parser.error("--spectrum-sketch-min-count: only with --spectrum-sketch")
                if not 1 <= args.spectrum_sketch_min_count < 2 ** 32:
                    parser.error("--spectrum-sketch-min-count: at least 1")
            if hasattr(args, "depth_filter"):
                from . import depth
                try:
                    args.depth_band = depth.parse_band(args.depth_filter)
                except ValueError as e:
                    parser.error(f"--depth-filter: {e}")
    if getattr(args, "gpu_png", False):
        if args.command == "query" and not args.keep_images:
            parser.error("--gpu-png: only with -m/--keep-images")
        if args.command == "query" and args.images:
            parser.error("--gpu-png: not with -I/--images (no image is made)")
        if args.command == "image" and args.no_image:
            parser.error("--gpu-png: not with -X/--no-image")
    if getattr(args, "gpu_png_read", False) and args.command == "query" and not args.images:
        parser.error("--gpu-png-read: only with -I/--images")
    if args.command in ("image", "query"):
        given = [flag for name, flag in ADAPTER_FLAGS if hasattr(args, name)]
        if given and not (args.from_raw or from_bam):
            parser.error(f"{', '.join(given)}: only with --from-raw (or --from-bam)")
        if given and args.no_adapter:
            parser.error(f"{', '.join(given)}: not with -a/--no-adapter")
        from .adapters import parse_adapter
        for name, flag in ADAPTER_FLAGS[1:]:
            if hasattr(args, name):
                try:
                    setattr(args, name, parse_adapter(getattr(args, name)))
                except ValueError as e:
                    parser.error(f"{flag}: {e}")
    return args


def run_convert(args):
    from .convert import convert_folder
    n = convert_folder(args.input, args.outdir, args.output_mapping, args.input_mapping, args.kmer_size,
                       args.sum_reverse_complements, args.overwrite, max(1, args.n_threads))
    eprint(f"Converted {n} images; written to {args.outdir}")


def draw_seeds(samples, seed):
    """{sample: seed}: str(row index) + str(random integer), one draw per sample in row order (image.py:1017) --
    drawn for every sample on every rank."""
    import numpy as np
    rng = np.random.default_rng(seed)
    return {s: int(str(i) + str(rng.integers(low=0, high=2 ** 32))) % (1 << 63) for i, s in enumerate(samples)}


def max_bp_of(args):
    """-M: '0' = all of the data (cli.py:496-501)."""
    return None if str(args.max_bp) == "0" else parse_size(args.max_bp)


def clean_options(args):
    """The cleaning flags of `--from-raw` (-T, -a, -r, -D and the adapters by sequence: absent = off) as
    pipeline.raw_to_images and raw_to_query take them."""
    front, tail = (int(x) for x in str(args.trim_bp).split(","))
    a1, a2 = getattr(args, "adapter_sequence", None), getattr(args, "adapter_sequence_r2", None)
    return dict(trim=(front, tail), adapter=not args.no_adapter, merge=not args.no_merge, dedup=not args.no_deduplicate,
                adapters=(a1, a2) if a1 is not None or a2 is not None else None,
                detect_adapters=getattr(args, "detect_adapters", False))


def clean_read_files(src):
    """The cleaned read files of `src` (of its clean_reads/, when it is an intermediate folder), sorted."""
    src = Path(src)
    if (src / "clean_reads").is_dir():
        src = src / "clean_reads"
    return sorted(f for f in src.iterdir() if f.is_file() and f.name.endswith((".fq", ".fq.gz", ".fastq", ".fastq.gz")))


def run_query(args):
    """`varKoder query` from step C on (commands/query.py:188-324): images are made on the GPU and
    stay there for the model's input transform; predictions.csv has the reference's columns.  With --from-raw from
    step B on, like the reference's own default (prepare_images, :97-178): the input is listed by
    rawinput.process_input(is_query=True), cleaned, subsampled once and counted by pipeline.raw_to_query, and each
    row carries what its image's text chunks would hold (label `query`, the sample's base-frequency sd).  The
    reference writes no stats.csv for a query; neither does this.
    Under a launcher (one process per GPU) the inputs are sharded by size over the ranks (shard.shard_by_size) -- every rank
    makes its images and runs the model on its GPU -- and rank 0 writes predictions.csv in input order
    (BASELINE config 5: images + batched inference on 8 GPUs; no data-path collective, one object gather)."""
    import io
    import numpy as np
    import torch
    from PIL import Image
    from . import query as Q
    from .convert import get_metadata_from_img_filename
    from .engine import ImageEngine
    from .image import png_head, stem, write_png, write_png_parts
    from .pipeline import clean_to_query
    from .pngread import read_file, read_images
    from .shard import agreed_weights, io_threads_per_rank, shard_by_size, world_info
    from .subsample import split_name
    rank, world, device = world_info()
    outdir = Path(args.outdir)
    if not args.overwrite and (outdir / "predictions.csv").exists():
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")
    from_raw = getattr(args, "from_raw", False) or getattr(args, "from_bam", False)   # (--from-bam: RawPlan lists BAM files)
    from_fasta = getattr(args, "from_fasta", False)
    if from_fasta:
        from .fasta import fasta_files, fasta_to_query, sample_of
        inputs = fasta_files(args.input)
    elif args.images:
        inputs = sorted(Path(args.input).rglob("*.png"))
    elif from_raw:
        inputs = RawPlan(args, is_query=True)   # (no collective in it, nothing on the GPU: an input error leaves every rank here)
    else:
        inputs = clean_read_files(args.input)
    if not inputs:
        raise Exception("No images found to query. Please check your input.")
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)        # control plane only
    # A rank that fails must not leave the others waiting in the gather: its work runs inside one try block, the
    # error travels WITH the gathered results, and every rank -- failed or not -- takes part in the gather and the
    # closing barrier; the exception is raised after the process group is gone.
    state = {"eng": None}
    model = vocab = None
    # (collectives: outside the try block, every rank is still here)
    if from_raw:
        raw_weights, clean_weights = inputs.agree_weights()
    else:
        weights = agreed_weights(inputs)

    def rank_work():
        nonlocal model, vocab
        model, vocab = Q.load_model(args.model), Q.read_vocab(args.vocab)
        records, images, order = [], None, []   # order: index of each record's input in `inputs`
        eng = None
        mine = [] if from_raw else shard_by_size(weights, rank, world)

        def found_images(found, wanted, labels):
            """Records (in the order of wanted = [(index in `inputs`, sample)]), stacked images and kept PNGs of the
            samples that found = {sample: (bp, histogram, sd)} holds; labels: {sample: [labels]}."""
            hists, keep = [], []
            for i, sample in wanted:
                if sample not in found:
                    continue
                bp, hist, sd = found[sample]
                name = split_name(sample, bp) + f"+{args.kmer_mapping}+k{args.kmer_size}.png"
                path = str(outdir / "query_images" / name) if args.keep_images else name
                # what write_png puts into the image's text chunks, read back as a query of that image reads it
                text, qual, freq_sd = Q.image_metadata({"varkoderKeywords": LABELS_SEP.join(labels.get(sample, [])),
                                                        "varkoderBaseFreqSd": str(sd),
                                                        "varkoderLowQualityFlag": str(sd > QUAL_THRESH)})
                records.append(dict(path=path, sample=sample, bp=int(bp / 1000) * 1000, k=args.kmer_size,
                                    mapping=args.kmer_mapping, labels=text, qual=qual, freq_sd=freq_sd))
                hists.append(hist)
                keep.append((name, sample, sd))
                order.append(i)
            if not hists:
                return None
            images = eng.images(torch.stack(hists))
            if args.keep_images:
                (outdir / "query_images").mkdir(parents=True, exist_ok=True)
                gpu_png = getattr(args, "gpu_png", False)
                host = eng.png(images) if gpu_png else images.cpu().numpy()
                for j, (name, sample, sd) in enumerate(keep):
                    text = (labels.get(sample, []), sd, QUAL_THRESH, args.kmer_mapping)
                    if gpu_png:
                        write_png_parts(outdir / "query_images" / name, png_head(eng.side, *text), host[j])
                    else:
                        write_png(host[j], outdir / "query_images" / name, *text)
            return images

        if from_raw:
            eng = state["eng"] = ImageEngine(k=args.kmer_size, mapping=args.kmer_mapping, device=device)
            found = inputs.run(eng, raw_weights, clean_weights, rank, world)
            images = found_images(found, enumerate(inputs.samples), inputs.labels)
        elif args.images:
            arrays, datas = [], []
            gpu_read = getattr(args, "gpu_png_read", False)
            for i in mine:
                p = inputs[i]
                if gpu_read:   # the file's bytes once; PIL reads the chunks in front of the pixels from them, lazily as ever
                    datas.append(read_file(p))
                    im = Image.open(io.BytesIO(datas[-1]))
                else:
                    im = Image.open(p)
                md = get_metadata_from_img_filename(p)
                labels, qual, sd = Q.image_metadata(im.info)
                records.append(dict(path=str(p), sample=md["sample"], bp=md["bp"], k=md["img_kmer_size"],
                                    mapping=md["img_kmer_mapping"], labels=labels, qual=qual, freq_sd=sd))
                if not gpu_read:
                    arrays.append(np.array(im))
                order.append(i)
            shapes = {a.shape for a in arrays}
            if len(shapes) > 1:
                raise Exception("Images of different sizes in one query are not supported.")
            if arrays:
                eng = state["eng"] = ImageEngine(k=records[0]["k"], mapping="cgr", device=device)
                images = torch.from_numpy(np.stack(arrays)).to(eng.device)
            elif datas:
                eng = state["eng"] = ImageEngine(k=records[0]["k"], mapping="cgr", device=device)
                images = read_images(eng, [inputs[i] for i in mine], datas=datas,
                                     mixed="Images of different sizes in one query are not supported.")
        elif from_fasta:
            # a sample per FASTA file, imaged whole: rows as for cleaned reads (no labels, no base-frequency sd)
            if mine:
                eng = state["eng"] = ImageEngine(k=args.kmer_size, mapping=args.kmer_mapping, device=device)
                wanted = [(i, sample_of(inputs[i])) for i in mine]
                record_opts, origin = {}, {}
                if getattr(args, "per_record", False):
                    record_opts = dict(per_record=True, origin=origin,
                                       min_record_length=getattr(args, "min_record_length", MIN_RECORD_LENGTH_DEFAULT))
                if getattr(args, "windows", False):
                    record_opts = dict(origin=origin, **window_options(args))
                found = fasta_to_query([(s, inputs[i]) for i, s in wanted], engine=eng, k=args.kmer_size,
                                       mapping_code=args.kmer_mapping, io_threads=io_threads_per_rank(args.n_threads),
                                       genome=genome_spectrum_options(args), **record_opts)
                if record_opts:   # a row per record (or window), in the order of the files and of the records within each
                    of_file = {s: [] for _, s in wanted}
                    for rs in found:
                        of_file[origin[rs]].append(rs)
                    wanted = [(i, rs) for i, s in wanted for rs in of_file[s]]
                images = found_images(found, wanted, {})
        else:
            # cleaned reads, a sample per file: no labels and no base-frequency sd, as images written with neither read back
            max_bp = max_bp_of(args)
            seeds = draw_seeds([stem(f) for f in inputs], args.seed)
            if mine:
                eng = state["eng"] = ImageEngine(k=args.kmer_size, mapping=args.kmer_mapping, device=device)
                wanted = [(i, stem(inputs[i])) for i in mine]
                found = clean_to_query([(s, inputs[i]) for i, s in wanted], max_bp=max_bp, seeds=seeds, engine=eng,
                                       k=args.kmer_size, mapping_code=args.kmer_mapping,
                                       io_threads=io_threads_per_rank(args.n_threads), screen=screen_options(args),
                                       qc_dir=qc_options(args), spectrum=spectrum_options(args))
                images = found_images(found, wanted, {})
        if rank == 0:
            if args.single_label:
                eprint("This is a single label classification model, each input may will have only one prediction.")
            else:
                eprint("This is a multilabel classification model, each input may have 0 or more predictions.")
        probs = None
        if images is not None:
            probs = Q.probabilities(eng, images, model, batch_size=args.max_batch_size, multilabel=not args.single_label,
                                    input_size=args.input_size, half=args.half)
        return order, records, None if probs is None else np.asarray(probs)

    failure = None
    try:
        part = rank_work() + (None,)
    except Exception as e:   # noqa: BLE001 -- reported below, once every rank is past its collectives
        failure = e
        part = ([], [], None, "rank %d: %r" % (rank, e))
    parts = [part]
    if world > 1:
        import torch.distributed as dist
        bucket = [None] * world if rank == 0 else None
        dist.gather_object(part, bucket, dst=0)
        parts = bucket if rank == 0 else []
    if rank == 0:
        errors = [e for _, _, _, e in parts if e]
        try:
            if errors:
                raise failure if failure is not None else Exception("query failed on " + "; ".join(errors))
            rows = sorted(((i, r, p) for o, rs, ps, _ in parts if ps is not None for i, r, p in zip(o, rs, ps)), key=lambda t: t[0])
            if not rows:
                raise Exception("No images found to query. Please check your input.")
            df = Q.predictions_frame([r for _, r, _ in rows], np.stack([p for _, _, p in rows]), vocab, args.model,
                                     args.threshold, not args.single_label, args.include_probs)
            outdir.mkdir(parents=True, exist_ok=True)
            df.to_csv(outdir / "predictions.csv", index=False)
            eprint("Predictions saved to", str(outdir / "predictions.csv"))
        except Exception as e:   # noqa: BLE001
            failure = e
    if state["eng"] is not None:
        state["eng"].close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if failure is not None:
        raise failure


class RawPlan:
    """What `image --from-raw` and `query --from-raw` work on: the input table (rawinput.process_input), the labels
    and one seed per sample in table order (draw_seeds), and which samples an earlier run with the same -i has
    cleaned already.  len() = the samples."""

    def __init__(self, args, is_query):
        from .rawinput import process_input
        src = Path(args.input)
        if is_query and list(src.glob("*.png")):                              # query.py:111-120
            eprint("ERROR: Found PNG files in input directory.")
            eprint("If your input directory contains pre-generated images, use the --images flag:")
            eprint("    varkoder_amd query --images " + str(src) + " " + str(args.outdir))
            raise Exception("Input directory contains PNG files. Use --images flag for pre-generated images.")
        self.bam = bam_options(args)
        if self.bam is not None:   # every *.bam of the folder is one sample; labels as for --from-fasta
            from .bam import bam_files, sample_of
            files = bam_files(src)
            labels = {} if is_query else read_labels(getattr(args, "labels_csv", None))
            if self.bam["groups"] is not None:   # every read group of every file is one sample; a label by group sample first, then by its file's
                from .bam import group_samples
                from .fasta import RecordLabels
                members, why = group_samples(files)
                for f, reason in why.items():
                    eprint(f"{f}: {reason}")
                labels = RecordLabels(labels, [sample_of(f) for f in files])
                table = [(s, ["query"] if is_query else labels.get(s, []), [f]) for s, f, _ in members]
                self.bam["groups"] = {s: g for s, _, g in members}
            else:
                table = [(sample_of(f), ["query"] if is_query else labels.get(sample_of(f), []), [f]) for f in files]
        else:
            table = process_input(args.input, is_query=is_query)
        self.args = args
        self.samples = [s for s, _, _ in table]
        self.labels = {s: lab for s, lab, _ in table}   # (a query's: ["query"])
        self.seeds = draw_seeds(self.samples, args.seed)
        self.clean_dir = Path(args.int_folder) / "clean_reads" if args.int_folder else None
        # a cleaned file from an earlier run is used as it is (clean_reads, commands/image.py:350-352)
        reuse = {s for s in self.samples
                 if self.clean_dir is not None and not args.overwrite and (self.clean_dir / (s + ".fq.gz")).is_file()}
        for s in sorted(reuse):
            eprint("Skipping cleaning for", s + ":", "File exists.")
        self.raw = [(s, files) for s, _, files in table if s not in reuse]
        self.reused = sorted(reuse)

    def __len__(self):
        return len(self.samples)

    def reused_files(self):
        return [self.clean_dir / (s + ".fq.gz") for s in self.reused]

    def agree_weights(self):
        """(weight of each raw sample -- the sum of its files' --, weight of each reused cleaned file) as every rank
        uses them: collectives, raw first, none for an empty list."""
        from .pipeline import sample_weights
        from .shard import agreed_weights, world_info
        done = self.reused_files()
        return sample_weights(self.raw, world_info()[1]), (agreed_weights(done) if done else [])

    def run(self, eng, raw_weights, clean_weights, rank, world):
        """A query's {sample: (bp, histogram on the device, base-frequency sd)} of this rank's share."""
        from .image import base_sd_table
        from .pipeline import clean_to_query, raw_to_query
        from .shard import io_threads_per_rank, shard_by_size
        args = self.args
        common = dict(k=args.kmer_size, mapping_code=args.kmer_mapping, max_bp=max_bp_of(args), seeds=self.seeds, engine=eng,
                      io_threads=io_threads_per_rank(args.n_threads), screen=screen_options(args), qc_dir=qc_options(args),
                      spectrum=spectrum_options(args))
        found = {}
        if self.raw:
            found.update(raw_to_query(self.raw, weights=raw_weights, rank=rank, world=world, clean_dir=self.clean_dir,
                                      verbose=args.verbose, gpu_gzip=getattr(args, "gpu_gzip", False), bam=self.bam,
                                      **clean_options(args), **common))
        mine = [self.reused[i] for i in shard_by_size(clean_weights, rank, world)]
        if mine:
            found.update(clean_to_query([(s, self.clean_dir / (s + ".fq.gz")) for s in mine],
                                        base_sd=base_sd_table(self.clean_dir, mine), **common))
        return found


def read_labels(path):
    import pandas as pd
    if not path:
        return {}
    df = pd.read_csv(path, dtype=str).fillna("")
    return {r["sample"]: [x for x in r["labels"].split(LABELS_SEP) if x] for _, r in df.iterrows()}


def parse_size(text):
    """humanfriendly.parse_size for the forms the reference's flags take ("500K", "200M", "0"):
    decimal multiples, optional trailing B (commands/image.py:1013)."""
    t = str(text).strip().upper().removesuffix("B")
    mult = {"K": 10 ** 3, "M": 10 ** 6, "G": 10 ** 9, "T": 10 ** 12}
    if t and t[-1] in mult:
        return int(float(t[:-1]) * mult[t[-1]])
    return int(float(t))


def split_options(args):
    """--write-splits as pipeline.clean_to_images and raw_to_images take it: the folder, -x, and -X (honoured with the
    flag only: commands/image.py:1055)."""
    if not getattr(args, "write_splits", False):
        return {}
    return dict(split_dir=Path(args.int_folder) / "split_fastqs", overwrite=args.overwrite, no_image=args.no_image)


def run_image_from_clean(args, outdir, rank, world, local_rank):
    from .image import base_sd_table, stem
    from .pipeline import clean_to_images
    from .shard import agreed_weights, io_threads_per_rank
    files = clean_read_files(args.input)
    if not files:
        raise Exception("No files found in input. Please check.")
    samples = [stem(f) for f in files]
    max_bp = max_bp_of(args)
    seeds = draw_seeds(samples, args.seed)
    labels = read_labels(args.labels_csv)
    base_sd = base_sd_table(files[0].parent, samples)                         # image.py:1094-1097
    eprint("Subsampling, counting kmers and creating images for", len(files), "samples")
    per_sample, error = OrderedDict(), None
    weights = agreed_weights(files)   # (a collective: before the try block, while every rank is still here)
    try:   # (a rank whose share fails still reaches the gather below: see finish_image_job)
        failpoint(rank)
        per_sample = clean_to_images(files, outdir, weights=weights, k=args.kmer_size, mapping_code=args.kmer_mapping,
                                     min_bp=parse_size(args.min_bp), max_bp=max_bp, seeds=seeds, labels=labels,
                                     base_sd=base_sd, **split_options(args), gpu_gzip=getattr(args, "gpu_gzip", False),
                                     device=local_rank, rank=rank, world=world, io_threads=io_threads_per_rank(args.n_threads),
                                     verbose=args.verbose, gpu_png=getattr(args, "gpu_png", False), screen=screen_options(args),
                                     qc_dir=qc_options(args), spectrum=spectrum_options(args))
        for s, v in per_sample.items():
            v["base_frequencies_sd"] = base_sd.get(s, 0)
    except Exception as e:   # noqa: BLE001 -- reported by finish_image_job, once every rank is past its collectives
        error = e
    finish_image_job(args, outdir, rank, world, per_sample, error, samples, labels, base_sd)


def run_image_from_fasta(args, outdir, rank, world, local_rank):
    """`image --from-fasta`: every FASTA file of the input folder is one sample, counted whole and imaged (fasta.py)."""
    from .fasta import fasta_files, fasta_to_images, sample_of
    from .shard import agreed_weights, io_threads_per_rank
    files = fasta_files(args.input)
    if not files:
        raise Exception("No files found in input. Please check.")
    samples = [sample_of(f) for f in files]
    labels = read_labels(args.labels_csv)
    eprint("Counting kmers and creating images for", len(files), "FASTA samples")
    ladder = {}
    per_record = getattr(args, "per_record", False)
    if per_record:   # a label by record sample first, then by the sample of its file
        from .fasta import RecordLabels
        labels = RecordLabels(labels, samples)
        ladder = dict(per_record=True, min_record_length=getattr(args, "min_record_length", MIN_RECORD_LENGTH_DEFAULT))
    if getattr(args, "windows", False):   # a label by window sample first, then by record sample, then by the sample of its file
        from .fasta import RecordLabels
        labels = RecordLabels(labels, samples, windows=True)
        ladder = window_options(args)
        per_record = True   # (a row per imaged window, as per imaged record)
    if getattr(args, "fragments", False):   # -m, -M and -R as for --from-clean
        ladder = dict(fragments=True, fragment_length=getattr(args, "fragment_length", FRAGMENT_LENGTH_DEFAULT),
                      min_bp=parse_size(args.min_bp), max_bp=max_bp_of(args), seeds=draw_seeds(samples, args.seed))
    per_sample, error = OrderedDict(), None
    weights = agreed_weights(files)   # (a collective: before the try block, while every rank is still here)
    try:   # (a rank whose share fails still reaches the gather below: see finish_image_job)
        failpoint(rank)
        per_sample = fasta_to_images(files, outdir, weights=weights, k=args.kmer_size, mapping_code=args.kmer_mapping,
                                     labels=labels, device=local_rank, rank=rank, world=world,
                                     io_threads=io_threads_per_rank(args.n_threads), verbose=args.verbose, gpu_png=getattr(args, "gpu_png", False),
                                     genome=genome_spectrum_options(args), **ladder)
        for v in per_sample.values():
            v["base_frequencies_sd"] = 0   # (no cleaning report: the flag is False, as for any sample without one)
    except Exception as e:   # noqa: BLE001 -- reported by finish_image_job, once every rank is past its collectives
        error = e
    # (per record: the samples are the imaged records, known once the ranks' stats are merged)
    finish_image_job(args, outdir, rank, world, per_sample, error, None if per_record else samples, labels, {})


def run_image_from_raw(args, outdir, rank, world, local_rank):
    """`image --from-raw`: steps B-E per sample (run_clean2img, commands/image.py:938-1127) with step B on the GPU."""
    from .image import base_sd_table
    from .pipeline import clean_to_images, raw_to_images
    from .shard import io_threads_per_rank
    plan = RawPlan(args, is_query=False)
    if not plan:
        raise Exception("No files found in input. Please check.")
    max_bp, cleaning = max_bp_of(args), clean_options(args)
    eprint("Cleaning reads, subsampling, counting kmers and creating images for", len(plan), "samples")
    per_sample, base_sd, error = OrderedDict(), {}, None
    weights, cw = plan.agree_weights()   # (collectives: before the try block, while every rank is still here)
    try:   # (a rank whose share fails still reaches the gather below: see finish_image_job)
        failpoint(rank)
        common = dict(k=args.kmer_size, mapping_code=args.kmer_mapping, min_bp=parse_size(args.min_bp), max_bp=max_bp,
                      seeds=plan.seeds, labels=plan.labels, device=local_rank, rank=rank, world=world,
                      io_threads=io_threads_per_rank(args.n_threads), verbose=args.verbose, **split_options(args),
                      gpu_gzip=getattr(args, "gpu_gzip", False), gpu_png=getattr(args, "gpu_png", False),
                      screen=screen_options(args), qc_dir=qc_options(args), spectrum=spectrum_options(args))
        if plan.raw:
            got, sds = raw_to_images(plan.raw, outdir, weights=weights, clean_dir=plan.clean_dir, bam=plan.bam, **cleaning,
                                     **common)
            per_sample.update(got)
            base_sd.update(sds)
        if plan.reused:
            sds = base_sd_table(plan.clean_dir, plan.reused)
            base_sd.update(sds)
            per_sample.update(clean_to_images(plan.reused_files(), outdir, weights=cw, base_sd=sds, **common))
        for s, v in per_sample.items():
            v["base_frequencies_sd"] = base_sd.get(s, 0)
    except Exception as e:   # noqa: BLE001 -- reported by finish_image_job, once every rank is past its collectives
        error = e
    # (--bam-read-groups: a group without reads is no sample; the samples are those that came through)
    grouped = plan.bam is not None and plan.bam["groups"] is not None
    finish_image_job(args, outdir, rank, world, per_sample, error, samples=None if grouped else plan.samples, labels=plan.labels,
                     base_sd=base_sd)


def failpoint(rank):
    """Test hook: VARKODER_AMD_FAULT=rank<r> makes rank r's share of an `image` job raise before it starts (the tests of
    the job's failure isolation need a rank that fails for a reason no input file carries: a device out of memory, a
    full disk)."""
    if os.environ.get("VARKODER_AMD_FAULT") == "rank%d" % rank:
        raise RuntimeError("injected fault on rank %d (VARKODER_AMD_FAULT)" % rank)


def finish_image_job(args, outdir, rank, world, per_sample, error, samples, labels, base_sd):
    """The closing half of `image` on every rank: gather the ranks' per-sample stats (and errors) on rank 0, write
    stats.csv / labels.csv there, meet at the barrier, leave the group -- and only then raise what went wrong.

    The reference's pool loses ONE sample when a worker dies on it (commands/image.py:1070-1075, :1281-1284); a job of
    ranks that share collectives loses every rank unless the failing one still shows up for them: an exception on one
    rank (the device out of memory in a copy, a PNG that cannot be written) used to leave the others inside
    gather_object until the gloo timeout.  Now the error travels with the gathered object, every rank reaches the
    gather and the barrier, rank 0 still writes the stats of what did finish, and every rank exits non-zero."""
    import pandas as pd
    from .shard import gather_stats
    text = None if error is None else "rank %d: %r" % (rank, error)
    merged, errors = gather_stats(per_sample, error=text, with_errors=True)
    failure = error
    if rank == 0:
        try:
            rows = [OrderedDict([("sample", s)] + list(v.items())) for s, v in merged.items()]
            pd.DataFrame(rows).to_csv(args.stats_file, index=False)
            if samples is None:   # `--from-fasta --per-record`, `--windows`: one row per imaged record or window
                samples = [s for s, v in merged.items() if "failed_step" not in v]
            if args.label_table and not errors:                               # image.py:1172-1185
                # (a sample of another rank whose figure only travelled with the stats: --from-raw computes it there)
                sd = {s: base_sd.get(s, merged.get(s, {}).get("base_frequencies_sd", 0)) for s in samples}
                lt = pd.DataFrame({"sample": samples,
                                   "labels": [LABELS_SEP.join(labels.get(s, [])) for s in samples],
                                   "possible_low_quality": [sd[s] > QUAL_THRESH for s in samples]})
                lt.to_csv(outdir / "labels.csv", index=False)
            if errors:
                eprint("image failed on", "; ".join(errors))
                if failure is None:
                    failure = Exception("image failed on " + "; ".join(errors))
            else:
                eprint("All images done, saved in", str(outdir))
        except Exception as e:   # noqa: BLE001
            failure = failure or e
    if world > 1:
        import torch.distributed as dist
        # every rank learns whether the job failed (a rank whose own share was fine must not report success)
        flag = [failure is not None]
        verdict = [None] * world
        dist.all_gather_object(verdict, flag[0])
        dist.barrier()
        dist.destroy_process_group()
        if failure is None and any(verdict):
            failure = Exception("image failed on another rank")
    if failure is not None:
        raise failure


def run_image(args):
    from .pipeline import fastqs_to_images
    from .shard import io_threads_per_rank, world_info
    if args.kmer_size not in range(KMER_MIN, KMER_MAX + 1):
        raise ValueError("kmer size must be between 5 and 9")               # image.py:1209-1210
    rank, world, local_rank = world_info()
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)        # control plane only
    outdir = Path(args.outdir)
    refuse = [False]
    if rank == 0:
        refuse[0] = (not args.overwrite) and outdir.exists()                # image.py:1219-1223
        if not refuse[0]:
            if outdir.is_dir():
                shutil.rmtree(outdir)
            outdir.mkdir(parents=True)
    if world > 1:
        dist.broadcast_object_list(refuse, src=0)   # every rank learns the verdict: nobody is left in a barrier
    if refuse[0]:
        if world > 1:
            dist.destroy_process_group()
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")
    if args.from_clean:
        return run_image_from_clean(args, outdir, rank, world, local_rank)
    if args.from_raw or getattr(args, "from_bam", False):   # (--from-bam: RawPlan lists BAM files, the run is the same)
        return run_image_from_raw(args, outdir, rank, world, local_rank)
    if getattr(args, "from_fasta", False):
        return run_image_from_fasta(args, outdir, rank, world, local_rank)
    src = Path(args.input)
    if (src / "split_fastqs").is_dir():
        src = src / "split_fastqs"
    files = sorted(f for f in src.iterdir() if SAMPLE_BP_SEP in f.name and f.is_file())
    if not files:
        raise Exception("No files found in input. Please check.")            # image.py:1309-1310
    samples = sorted({f.name.split(SAMPLE_BP_SEP)[0] for f in files})
    levels = math.floor(math.log(len(samples) / 1000, 16)) if samples else 0  # image.py:1246
    levels = max(levels, 0)
    labels = read_labels(args.labels_csv)
    from .image import base_sd_table
    # the fastp reports sit next to the split files in the intermediate folder (image.py:1094-1097)
    base_sd = base_sd_table(src.parent / "clean_reads", samples)
    eprint("varkoder_amd")
    eprint("Kmer size:", str(args.kmer_size))
    eprint("Counting kmers and creating images for", len(files), "files of", len(samples), "samples")
    if args.no_image:
        return
    mine, error = defaultdict(OrderedDict), None
    from .shard import agreed_weights
    weights = agreed_weights(files)   # (a collective: before the try block, while every rank is still here)
    try:   # (a rank whose share fails still reaches the gather: see finish_image_job)
        failpoint(rank)
        per_file = fastqs_to_images(files, outdir, weights=weights, k=args.kmer_size, mapping_code=args.kmer_mapping, labels=labels,
                                    base_sd=base_sd, overwrite=True, subfolder_levels=levels, device=local_rank, rank=rank,
                                    world=world, io_threads=io_threads_per_rank(args.n_threads), verbose=args.verbose,
                                    gpu_png=getattr(args, "gpu_png", False))
        # fold the per-file stats into per-sample stats like run_clean2img does (image.py:1057-1125); files are dealt by
        # size, so other ranks may hold further files of the same sample: shard.merge_stats adds the ranks' shares up
        ck, ik = f"{args.kmer_size}mer_counting_time", f"k{args.kmer_size}_img_time"
        if os.environ.get("VARKODER_AMD_PER_FILE_STATS"):   # (tests: this rank's per-file rows, before they are folded)
            import json
            with open(os.environ["VARKODER_AMD_PER_FILE_STATS"] + f".rank{rank}.json", "w") as f:
                json.dump(per_file, f)
        for key, st in per_file.items():
            s = mine[key.split(SAMPLE_BP_SEP)[0]]
            for name in (ck, ik):
                if name in st:
                    s[name] = s.get(name, 0) + st[name]
            if "failed_step" in st:
                s["failed_step"] = st["failed_step"]
        for name, st in mine.items():
            st["base_frequencies_sd"] = base_sd.get(name, 0)
    except Exception as e:   # noqa: BLE001 -- reported by finish_image_job, once every rank is past its collectives
        error = e
    finish_image_job(args, outdir, rank, world, mine, error, samples, labels, base_sd)


def main(argv=None):
    args = parse_args(argv)
    if not Path(args.input).exists():                                       # cli.py:503-505
        raise Exception("Input path", args.input, "does not exist. Please check.")
    if args.command in ("image", "query") and getattr(args, "from_bam", False) and getattr(args, "bam_pairs", False):
        # refused before anything is made or uploaded: mates of a file sorted by coordinate are not in the same order
        from .bam import bam_files, check_pairs
        why = check_pairs(bam_files(args.input)) if Path(args.input).is_dir() else None
        if why:
            eprint("error:", why)
            raise SystemExit(2)
    if args.command == "image":
        run_image(args)
    elif args.command == "convert":
        run_convert(args)
    elif args.command == "query":
        run_query(args)
    elif args.command == "train":
        from .train import run_train
        run_train(args)
    elif args.command == "compare":
        from .compare import run_compare
        run_compare(args)
    elif args.command == "distance":
        from .distance import run_distance
        run_distance(args)
    elif args.command == "tree":
        from .tree import run_tree
        run_tree(args)
    eprint("DONE")


if __name__ == "__main__":
    main(sys.argv[1:])
