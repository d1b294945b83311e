#!/usr/bin/env python
"""``bcftools isec -p DIR A B`` without bcftools: pairs the records of two position-sorted VCFs (plain, gzip or BGZF text)
by CHROM, POS, REF and the ALT set (isec's default ``-c none``) and writes

    DIR/0000.vcf  records private to A        DIR/0002.vcf  A's records shared with B
    DIR/0001.vcf  records private to B        DIR/0003.vcf  B's records shared with A

plus DIR/README.txt.  Each file has its input's header; record lines are copied byte for byte (bcftools re-prints them
through htslib and adds ##bcftools_isec lines: a documented, unpinned divergence).  A multi-allelic record pairs only with a
record of the same ALT set, so a truth ``A>G,T`` and a candidate ``A>G`` both stay private.  See dl4vc_amd/truthset.py.

    vcf_isec.py -p isec truth.vcf.gz candidates.vcf

``--left-align REF.fa`` (not a bcftools option): the simple indels of both inputs are moved to their left-most placement on the
FASTA before they are paired, so that one event named at two placements of a repeat pairs (dl4vc_amd/truthset.py::
left_align_record).  The lines written are still the inputs' own.

Every other bcftools isec option is refused, never ignored.
"""
from __future__ import annotations

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

USAGE = "usage: vcf_isec.py -p DIR [--left-align REF.fa] A.vcf[.gz] B.vcf[.gz]"


def parse_args(argv):
    prefix, files, left_align = None, [], None
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in ("-h", "--help"):
            print(__doc__)
            raise SystemExit(0)
        if a in ("-p", "--prefix"):
            if i + 1 >= len(argv):
                raise SystemExit("vcf_isec.py: %s needs a directory\n%s" % (a, USAGE))
            prefix = argv[i + 1]
            i += 2
            continue
        if a == "--left-align":
            if i + 1 >= len(argv):
                raise SystemExit("vcf_isec.py: --left-align needs the reference FASTA\n%s" % USAGE)
            left_align = argv[i + 1]
            i += 2
            continue
        if a.startswith("--left-align="):
            left_align = a[len("--left-align="):]
        elif a.startswith("--prefix="):
            prefix = a[len("--prefix="):]
        elif a.startswith("-p") and len(a) > 2:
            prefix = a[2:]
        elif a.startswith("-") and a != "-":
            raise SystemExit("vcf_isec.py: bcftools isec option %s is not supported: only -p DIR (the default collapse mode "
                             "-c none, all records, no filters) is implemented\n%s" % (a, USAGE))
        else:
            files.append(a)
        i += 1
    if prefix is None:
        raise SystemExit("vcf_isec.py: -p DIR is required (bcftools isec without -p prints a site list, which is not "
                         "implemented)\n%s" % USAGE)
    if len(files) != 2:
        raise SystemExit("vcf_isec.py: exactly two VCF files are needed, got %d\n%s" % (len(files), USAGE))
    if left_align is not None and not os.path.isfile(left_align):
        raise SystemExit("vcf_isec.py: --left-align %s is not a readable file" % left_align)
    return prefix, files[0], files[1], left_align


def main(argv=None):
    from dl4vc_amd.truthset import VcfError, isec_to_dir
    prefix, a, b, left_align = parse_args(sys.argv[1:] if argv is None else argv)
    t0 = time.time()
    try:
        counts = isec_to_dir(a, b, prefix, left_align=left_align)
    except VcfError as e:
        print("vcf_isec.py: %s" % e, file=sys.stderr)
        return 1
    print("vcf_isec.py: %d private to A, %d private to B, %d shared (%.1f s)" % (counts[0], counts[1], counts[2],
                                                                              time.time() - t0), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
