#!/usr/bin/env python3
"""Drop-in for the reference's ``main.py`` (main.py:47-229): inference-only mode (branch :213-222) and, with
``--train_file`` (or ``--train_bam``: the records encoded from the BAM on the GPU, no file), training + per-epoch evaluation
(branch :151-199).

    python main.py <the flags call_variants.sh passes> --test_file X.hdf --modelload CKPT \
        --save_vcf_records --save_vcf_records_file OUT/model_test.vcf --sample_vcf OUT/candidates.vcf

Reads the candidate HDF5 (schema of tools/convert_bam_single_reads.py), scores every site with the
MI355X-native DAN forward and writes ``OUT/epoch1_model_test.vcf`` exactly where and how the reference does
(dl4vc/utils.py:146-178).  ``--gpus N`` starts one process per GPU over contiguous site shards and
concatenates the part files on the host; there is no collective on this path.  With ``--train_file`` the flags of
train_variant_caller.sh:101-151 drive ``dl4vc_amd/trainer.py`` (one process per GPU, one RCCL all-reduce of the flat
gradient buffer per step); training options outside the published script's path are refused, never ignored.
"""
from __future__ import annotations

import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from arguments import parse_args                              # noqa: E402
from dl4vc_amd.procs import child_devices, wait_children      # noqa: E402,F401


def whole_lines(stream) -> None:
    """The ranks of a --gpus N run write to one stdout.  Where Python writes it through (``python -u``, PYTHONUNBUFFERED), ``print``
    hands a line's text and its line end to the pipe one after the other, and another rank's line can land between the two: two
    lines on one, an empty one behind them.  Buffered up to the next flush -- what a pipe gets by default -- a line goes out in
    one piece; every line a reader looks for here is printed with ``flush=True``."""
    if getattr(stream, "write_through", False):
        try:
            stream.reconfigure(write_through=False)
        except (AttributeError, ValueError, OSError):
            pass


def train_main(args, argv) -> int:
    """main.py:60-80,114-117,151-199: train for --epochs, evaluate on --test_file after every epoch, save checkpoints."""
    import numpy as np
    train_bam = getattr(args, "train_bam", None)
    if not train_bam:
        assert args.train_file[-3:] == "hdf", "Train dataset must be in HDF format"               # main.py:66
    if args.test_file:
        assert args.test_file[-3:] == "hdf", "Test dataset must be in HDF format"
    refused = [("--augment-single-reads", args.augment_single_reads), ("--augment-reference", args.augment_reference),
               ("--rm_var_reads_rate", args.rm_var_reads_rate > 0),
               ("--rm_non_var_reads_rate", args.rm_non_var_reads_rate > 0),
               ("--training_use_directional_augmentation", args.training_use_directional_augmentation),
               ("--train-trust-region-table", bool(args.train_trust_region_table)), ("--gatk-table", bool(getattr(args, "gatk_table", "")))]
    bad = [n for n, on in refused if on]
    if bad:
        raise SystemExit("training option(s) %s are not supported (off in train_variant_caller.sh:101-151): refusing rather than "
                         "silently training something else" % ", ".join(bad))
    if args.precision != "fp32":
        raise SystemExit("training runs in fp32 only")
    train_source, test_source = args.train_file, args.test_file
    if train_bam:
        train_source, test_source = bam_sources(args)         # (VCFs that cannot be read end the run here, before any device work)
    from dl4vc_amd.config import DanConfig
    device_loader = args.train_loader_device == "gpu"
    if device_loader:
        # a file the device loader cannot take is refused before anything starts, with the device loader's own reasons
        from dl4vc_amd.chunk_loader import check_layout
        from dl4vc_amd.hdf5io import RawChunkFile
        try:
            for path in (args.train_file, args.test_file):
                if not path:
                    continue                                  # (--train_bam / --test_bam stand in for it)
                with RawChunkFile(path) as raw:
                    check_layout(raw, DanConfig.from_args(args).reads)
        except (ValueError, RuntimeError, OSError, KeyError) as e:
            raise SystemExit("--train-loader-device gpu: %s" % e)
        # the loader shares device buffers and streams with torch: torch's HIP runtime has to be the process's only one, so it
        # is loaded before libdl4vc_dan.so brings in its own (as on --test_bam)
        import torch
        if args.gpus <= 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            if not torch.cuda.is_available():
                raise SystemExit("--train-loader-device gpu needs a HIP device visible to torch; there is no CPU path")
    from dl4vc_amd.train import DanTrainer, TrainHyper
    from dl4vc_amd.model import load_checkpoint
    from dl4vc_amd import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        whole_lines(sys.stdout)                               # (the ranks share one stdout)
    if args.gpus > 1 and world == 1:
        # one process per GPU (the reference: one process, nn.DataParallel over args.gpus devices, main.py:117)
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        devices = child_devices(args.gpus)
        procs = []
        for g in range(args.gpus):
            env = dict(os.environ, HIP_VISIBLE_DEVICES=devices[g], HSA_ENABLE_IPC_MODE_LEGACY="0", RANK=str(g), WORLD_SIZE=str(args.gpus),
                       LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.pop("CUDA_VISIBLE_DEVICES", None)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
        rcs = wait_children(procs)
        if any(rcs):
            raise SystemExit("training rank failed: %s" % rcs)
        return 0
    dist = all_reduce = gather = exchange = None
    if world > 1:
        import torch
        import torch.distributed as dist
        backend = os.environ.get("DL4VC_DIST_BACKEND", "nccl")        # (tests rehearse two ranks on one GPU over gloo)
        torch.cuda.set_device(0)
        # second line of defence behind the sharded evaluation below: a rank may legitimately wait long for another (check-
        # point writes, uneven loader start-up), and the backend's default collective timeout (10 min on RCCL) would kill the run
        import datetime
        dist.init_process_group(backend, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=float(os.environ.get("DL4VC_DIST_TIMEOUT_S", "7200"))))
        all_reduce = dist.all_reduce
        from dl4vc_amd.train import GradientExchange
        exchange = GradientExchange(dist, world)                     # bucketed, overlapped with the backward pass

        def gather(item):
            out = [None] * world
            dist.all_gather_object(out, item)
            return out

    cfg = DanConfig.from_args(args)
    hyper = TrainHyper.from_args(args)
    print("Train on %d rank(s); lr %s, batch %d, dropout %s" % (world, hyper.lr, args.batch_size, hyper.dropout))
    if device_loader:
        print("--train-loader-device gpu: batches are assembled on the GPU by one loader thread per file; --num-data-workers %d "
              "starts no worker process" % args.num_data_workers)
    resident = getattr(args, "train_cache_device", None) == "gpu"
    record_format = getattr(args, "train_cache_format", "rows")
    cache = {"left": None}                               # bytes of the budget the files still to be opened may take
    per_rank = -(-args.batch_size // world)
    trainer = DanTrainer(cfg, hyper, max_batch=per_rank, device_id=0)
    if args.modelload:
        print("Loading model checkpoint from {}".format(args.modelload))
        trainer.load_state_dict(load_checkpoint(args.modelload))
    else:
        trainer.load_state_dict(synth.torch_default_init(cfg, seed=args.seed, dropout_keys=hyper.dropout > 0))
    from dl4vc_amd.train_data import BatchPrefetcher, DeviceBatchPrefetcher
    from dl4vc_amd.train_data import BatchError

    def budget():
        # one budget for the trimmed records of both files; by default three quarters of what is free now that the trainer has
        # allocated (it bounds the records' bytes: each file's last slab is allocated whole).  A fill from a BAM asks once its
        # staging planes are allocated, so that they are not counted as free
        if cache["left"] is None:
            import torch
            cache["left"] = getattr(args, "train_cache_bytes", 0) or torch.cuda.mem_get_info(0)[0] * 3 // 4
        return cache["left"]

    def open_loader(path, batch_sites):
        # loader workers (main.py:59-60: DataLoader(num_workers=args.num_data_workers)); 0 = assemble in this process
        from dl4vc_amd.chunk_loader import BamSource
        from_bam = isinstance(path, BamSource)
        if not from_bam and not device_loader:
            return BatchPrefetcher(path, args.num_data_workers)
        if not from_bam and not resident:
            try:
                return DeviceBatchPrefetcher(path, cfg.reads, batch_sites, device=0, use_q=cfg.use_q, use_strand=cfg.use_strand)
            except (ValueError, RuntimeError) as e:
                raise SystemExit("--train-loader-device gpu: %s" % e)
        t0 = time.time()
        try:
            # (a fill from a BAM asks for the budget itself, once its staging planes are allocated)
            loader = DeviceBatchPrefetcher(path, cfg.reads, batch_sites, device=0, use_q=cfg.use_q, use_strand=cfg.use_strand,
                                           resident=True, cache_bytes=budget if from_bam else budget(), record_format=record_format)
        except (ValueError, RuntimeError) as e:
            raise SystemExit("--train-cache-device gpu: %s" % e)
        cache["left"] -= loader.stage["store_bytes"]
        report_resident(path, loader, time.time() - t0)
        return loader

    try:
        train_loop(args, cfg, hyper, trainer, open_loader, per_rank, rank, world, dist, all_reduce, gather, exchange,
                   train_source, test_source)
    except BatchError as e:
        # a damaged chunk or a record the loader refuses: the reason, not a traceback (under --gpus N the parent ends the other
        # ranks as soon as this one has exited, ``procs.wait_children``)
        raise SystemExit("--train-loader-device gpu: %s" % e)
    trainer.close()
    if dist is not None:
        dist.destroy_process_group()
    return 0


def report_resident(source, loader, seconds):
    """The line of ``--train-cache-device gpu`` once a source (a candidate file's path or a ``BamSource``) is resident."""
    from dl4vc_amd.chunk_loader import BamSource
    from_bam = isinstance(source, BamSource)
    st, planes = loader.stage, loader.loader.inflated_bytes
    line = "--train-cache-device gpu: %s: %d records resident in %d bytes (%.3f of their %d %s bytes), filled in %.2f s" \
        % (source.bam if from_bam else source, st["store_records"], st["store_bytes"], st["store_bytes"] / max(1, planes), planes,
           "plane" if from_bam else "inflated", seconds)
    if loader.loader.record_format != "rows":
        line += "; --train-cache-format %s: %d records in %d bytes (%.3f of their %d %s bytes), %d records fell back to rows (%d bytes)" \
            % (loader.loader.record_format, st["store_compact_records"], st["store_compact_bytes"], st["store_compact_bytes"] / max(1, planes),
               planes, "plane" if from_bam else "inflated", st["store_rows_records"], st["store_rows_bytes"])
    if from_bam:
        line += "; %d locations: %d on the GPU, %d by pe_encode, %d by the Python builder, %d without a record" \
            % (st["locations"], st["gpu"], st["native"], st["python"], st["no_record"])
    print(line, flush=True)


class RecordCount:
    """What ``train_epoch`` and ``evaluate`` need of a source when a loader makes their batches: how many records there are."""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n


def bam_sources(args):
    """--train_bam -> (the training source, the evaluation source): ``chunk_loader.BamSource``s, or --test_file's path.  The
    locations are built as tools/convert_bam_single_reads.py builds them -- tp (label 0, with the full VCF's genotypes), fn (1), fp (2),
    in that order -- so record i is record i of the file the converter would write and draws its read subset with the same seed."""
    from dl4vc_amd.chunk_loader import BamSource
    from dl4vc_amd.pileup_encoder import locations_from_vcf
    get = lambda k: getattr(args, k, None)   # noqa: E731

    def labelled(prefix):
        locs = []
        if get(prefix + "_tp_vcf"):
            locs += locations_from_vcf(get(prefix + "_tp_vcf"), 0, get(prefix + "_tp_full_vcf"))
        if get(prefix + "_fn_vcf"):
            locs += locations_from_vcf(get(prefix + "_fn_vcf"), 1)
        if get(prefix + "_fp_vcf"):
            locs += locations_from_vcf(get(prefix + "_fp_vcf"), 2)
        return locs

    try:
        opt = bam_encoder_options(args)
        train = BamSource(args.train_bam, args.train_fasta, labelled("train"), inflate_device=args.inflate_device, encoder_options=opt)
        if not args.test_bam:
            return train, args.test_file
        if any(get("test_%s_vcf" % k) for k in ("tp", "fn", "fp")):
            locs = labelled("test")
        else:
            locs = locations_from_vcf(args.sample_vcf, label=2)   # (as in inference)
        return train, BamSource(args.test_bam, args.test_fasta, locs, inflate_device=args.inflate_device, encoder_options=opt)
    except (OSError, ValueError, IndexError) as e:
        raise SystemExit("--train_bam: the location VCFs could not be read: %s" % e)


def train_loop(args, cfg, hyper, trainer, open_loader, per_rank, rank, world, dist, all_reduce, gather, exchange,
               train_source=None, test_source=None) -> None:
    """The epochs of ``train_main``: train, decay the learning rate, evaluate, save.  ``train_source`` / ``test_source``:
    --train_file's and --test_file's paths (the default), or the ``BamSource``s of --train_bam / --test_bam -- then the resident
    records give the record count and the chromosomes that a file gives otherwise."""
    import contextlib
    import numpy as np
    from dl4vc_amd.trainer import train_epoch, evaluate, save_checkpoint, checkpoint_state
    from dl4vc_amd.train_data import EasyExampleSampler
    from dl4vc_amd.hdf5io import CandidateFile
    from dl4vc_amd.model import DanNet
    from dl4vc_amd.vcf import start_scored_vcf, scored_vcf_path
    from dl4vc_amd.inference import select_records, select_sites
    from dl4vc_amd.shard import check_replicas_agree
    best_loss = None
    train_source = args.train_file if train_source is None else train_source
    test_source = args.test_file if test_source is None else test_source
    with contextlib.ExitStack() as stack:
        on_file = [isinstance(s, str) for s in (train_source, test_source)]
        train_src = stack.enter_context(CandidateFile(train_source)) if on_file[0] else None
        test_src = stack.enter_context(CandidateFile(test_source)) if on_file[1] else None
        train_loader = stack.enter_context(open_loader(train_source, per_rank))
        test_loader = stack.enter_context(open_loader(test_source, args.test_batch_size))
        if train_src is None:
            train_src = RecordCount(len(train_loader))
        if test_src is None:
            test_src = RecordCount(len(test_loader))

        def held_out(source, loader, chromosomes):
            if isinstance(source, str):
                return select_sites(source, chromosomes)
            return select_records(loader.loader.chromosomes(), chromosomes)

        holdout = None
        if args.train_holdout_chromosomes:
            holdout = np.zeros(len(train_src), bool)
            holdout[held_out(train_source, train_loader, args.train_holdout_chromosomes)] = True
        # every rank draws the same epoch order (same seed) and takes its DataParallel-style share of every batch
        plain = args.close_examples_sample_rate >= 1.0                # main.py:72-77: then a plain shuffled loader, no sampler
        if plain:
            print("keeping all examples -- no close example down-sampling")
            if holdout is not None and holdout.any():
                print("WARNING: as in the reference (main.py:75-77), without the easy-example sampler the %d held-out sites are NOT "
                      "skipped; use --close_examples_sample_rate < 1 to hold them out" % int(holdout.sum()))
        sampler = EasyExampleSampler(len(train_src), close_keep=min(1.0, args.close_examples_sample_rate), holdout=holdout,
                                     rng=np.random.RandomState(args.seed), plain=plain)
        test_idx = held_out(test_source, test_loader, args.test_holdout_chromosomes) if args.test_holdout_chromosomes else None
        for epoch in range(1, args.epochs + 1):
            s = time.time()
            print("Train Epoch: %d lr: [%s] on %d GPUs!" % (epoch, trainer.hyper.lr, world))
            train_epoch(trainer, train_src, sampler, hyper, args.batch_size, epoch, reads_seed=args.reads_seed,
                        max_batches=args.max_train_batches, keep_candidate_af=args.aux_keep_candidate_af, rank=rank, world=world,
                        all_reduce=all_reduce, gather=gather, exchange=exchange, prefetcher=train_loader,
                        log_interval=args.log_interval,
                        log=lambda m: print(m, end="\r"),
                        # (dataset.py:531; --delay_augmentation_epochs gates the directional augmentation only, main.py:161-165)
                        downsample_rate=args.reads_dynamic_downsample_rate, downsample_prob=args.reads_dynamic_downsample_prob)
            print("\n\tTime elapsed for training {:.4f}\n".format(time.time() - s), flush=True)
            s_eval = time.time()
            trainer.set_lr(trainer.hyper.lr * args.lr_decay)                                      # main.py:166
            if epoch <= args.epochs_skip_eval:
                print("Skipping eval for epoch %d" % epoch)
                continue
            # evaluation is SHARDED over the ranks (the reference evaluates under the same DataParallel model, trainer.py:509-681):
            # rank r scores a contiguous run of the test batches with the parameters every rank holds (rank 0's BatchNorm
            # running statistics, broadcast -- DataParallel keeps replica 0's), the loss sums are reduced, the record text is
            # concatenated in rank order = batch order.  No rank idles in a barrier while rank 0 walks a genome-scale file.
            # Only the BatchNorm running statistics can differ between ranks (parameters are identical behind the averaged step;
            # statistics are per replica): those few vectors are broadcast, not the pickled 311-MB state dict.
            state = trainer.state_dict()
            if dist is not None:
                import torch
                on_gpu = dist.get_backend() == "nccl"

                def all_reduce_max(vec):
                    t = torch.from_numpy(np.asarray(vec, np.float64).copy())
                    if on_gpu:
                        t = t.cuda()
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    return t.cpu().numpy()
                # the assumption the broadcast below rests on, checked: one all-reduce of six numbers per evaluation
                check_replicas_agree(state, all_reduce_max, "epoch %d evaluation" % epoch)
                for key in sorted(k for k in state if k.startswith("bn1D_layers.") and
                                  k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")):
                    v = np.ascontiguousarray(state[key])
                    t = torch.from_numpy(v.copy())
                    if on_gpu:
                        t = t.cuda()
                    dist.broadcast(t, src=0)
                    state[key] = t.cpu().numpy().astype(v.dtype).reshape(v.shape)
            net = DanNet(cfg, device_id=0, max_batch=args.test_batch_size).load_state_dict(state)
            out_path = None
            if args.save_vcf_records:
                assert args.save_vcf_records_file != "", "Need a valid filename for args.save_vcf_records_file to save records"
                out_path = scored_vcf_path(args.save_vcf_records_file, epoch)
            part = (out_path + ".part%d" % rank) if (out_path and world > 1) else None
            out = None
            if out_path and rank == 0:
                if args.sample_vcf:
                    start_scored_vcf(args.sample_vcf, args.save_vcf_records_file, epoch)
                else:
                    open(out_path, "w").close()
            if out_path:
                out = open(part, "w") if part else open(out_path, "a")
            loss_sum, n_eval = evaluate(net, test_src, hyper, args.test_batch_size, write=out.write if out else None,
                                        reads_seed=args.reads_seed, max_batches=args.max_test_batches, indices=test_idx,
                                        prefetcher=test_loader, rank=rank, world=world, reduce=False)
            if out:
                out.close()
            net.close()
            if dist is not None:
                import torch
                t = torch.tensor([loss_sum, float(n_eval)], dtype=torch.float64,
                                 device="cuda" if dist.get_backend() == "nccl" else "cpu")
                dist.all_reduce(t)
                loss_sum, n_eval = float(t[0]), int(t[1])
            curloss = loss_sum / max(n_eval, 1)
            if rank == 0:
                if part:
                    with open(out_path, "a") as dst:
                        for r in range(world):
                            with open(out_path + ".part%d" % r) as src:
                                dst.write(src.read())
                            os.remove(out_path + ".part%d" % r)
                print("\nTest set: Average loss: {:.6f}\n".format(curloss))
                is_best = best_loss is None or curloss < best_loss
                best_loss = curloss if best_loss is None else min(curloss, best_loss)
                save_checkpoint(checkpoint_state(trainer, epoch, best_loss), is_best, args.modelsave)   # main.py:194-199
            print("\tTime elapsed for inference/testing {:.4f}".format(time.time() - s_eval))
            print("\tTime elapsed overall {:.4f}\n".format(time.time() - s), flush=True)
            if dist is not None:
                dist.barrier()
        for name, l in (("training", train_loader), ("evaluation", test_loader)):
            if hasattr(l, "stage") and rank == 0:
                print("device loader (%s file): %s" % (name, ", ".join("%s %s" % (k, ("%.1f" % v) if k.endswith("_ms") else int(v))
                                                                          for k, v in l.stage.items())))


GPUS_WITH_BAM = ("--test_bam runs on one GPU: a shard's read subsets are seeded with the index of its first RECORD, which needs the "
                 "number of locations without a record in every shard before it; drop --gpus, or convert to candidates.hdf "
                 "(tools/convert_bam_single_reads.py) and use --test_file --gpus N; or count the records first with --record-census gpu")
CENSUS_SIBLINGS = "DL4VC_CENSUS_SIBLINGS"      # set by the --gpus parent: the shards census a slice each and exchange side files


def check_bam_arguments(args) -> None:
    """--test_bam: what it needs and what it refuses (nothing is silently ignored)."""
    if args.test_file:
        raise SystemExit("--test_file and --test_bam are two sources of the same sites: give exactly one")
    if args.train_file:
        raise SystemExit("--test_bam is an inference input; training from a --train_file evaluates on a --test_file (--train_bam takes a "
                         "--test_bam beside it)")
    if not args.test_fasta or not args.sample_vcf:
        raise SystemExit("--test_bam needs --test_fasta (the reference) and --sample_vcf (the candidate VCF: its records are the sites)")
    if args.record_census:
        return                                                # (the census gives every record's index: shards and holdout are planned from it)
    if args.gpus > 1 or args.shard:
        raise SystemExit(GPUS_WITH_BAM)
    if args.test_holdout_chromosomes:
        raise SystemExit("--test_holdout_chromosomes is not supported with --test_bam: on a candidate file the held-out records keep "
                         "the record index (the read-subset seed) they have among ALL records, which only encoding every location "
                         "would give; filter the candidate VCF instead, or count the records first with --record-census gpu")


def census_text(st) -> str:
    """The census figures of a shard's statistics, for its line; "" for a shard without a census."""
    if "census_s" not in st:
        return ""
    return ("; census_s %.2f for %d locations (%d records; census_ms %.1f on the device), census_wait_s %.2f for the other shards"
            % (st["census_s"], st.get("census_locations", 0), st.get("census_records", 0), st.get("census_ms", 0.0),
               st.get("census_wait_s", 0.0)))


def score_bam_census(args, net, target, out_final, shard_i, shard_n, holdout, site_limit, stats, counts, census_stats, score_stage=None) -> int:
    """--test_bam --record-census gpu: census, plan (``shard.plan_bam_shard``), score this shard's runs into ``target``.
    Under a --gpus parent the shards census a contiguous slice of ALL locations each and exchange the flags through side files
    next to their parts; a --shard without siblings, and a run without shards, censuses every location itself."""
    import numpy as np
    from dl4vc_amd.inference import census_bam, score_bam
    from dl4vc_amd.pileup_encoder import locations_from_vcf
    from dl4vc_amd.shard import census_path, plan_bam_shard, shard_range, wait_census, write_census
    locations = locations_from_vcf(args.sample_vcf, label=2)
    siblings = int(os.environ.get(CENSUS_SIBLINGS, "0") or 0)
    if siblings and siblings != shard_n:
        raise SystemExit("%s=%d but --shard %s" % (CENSUS_SIBLINGS, siblings, args.shard))
    lo, hi = shard_range(len(locations), shard_i, shard_n) if siblings else (0, len(locations))
    if shard_n > 1 and not siblings:
        print("--shard %d/%d without sibling processes: this process censuses all %d locations itself" % (shard_i, shard_n, len(locations)))
    stage = {}
    t0 = time.time()
    opt = bam_encoder_options(args)
    sub = {"encoder_options": opt} if opt is not None else {}     # (without --subsample or a read filter the calls are what they were)
    mine = census_bam(args.test_bam, args.test_fasta, locations[lo:hi], inflate_device=args.inflate_device, stage=stage,
                      log=lambda m: print(m, end="\r"), **sub)
    census_stats.update(census_s=time.time() - t0, census_ms=float(stage.get("census_ms", 0.0)), census_locations=hi - lo,
                        census_records=int(mine.sum()), census_wait_s=0.0)
    if siblings:
        write_census(census_path(out_final, shard_i), mine)
        t1 = time.time()
        try:
            flags = wait_census(out_final, shard_n, [b - a for a, b in (shard_range(len(locations), g, shard_n) for g in range(shard_n))],
                                timeout_s=args.census_timeout)
        except RuntimeError as e:
            raise SystemExit("--record-census gpu: %s" % e)
        census_stats["census_wait_s"] = time.time() - t1
    else:
        flags = mine
    held = None
    if holdout:
        want = set(holdout)                                   # (select_sites: the text before the record's first tab)
        held = np.fromiter((l.vcf_string.split("\t", 1)[0] in want for l in locations), bool, len(locations))
    runs = plan_bam_shard(flags, held, site_limit, shard_i, shard_n)
    n = 0
    with open(target, "w") as f:
        for a, b, first in runs:
            n += score_bam(net, args.test_bam, args.test_fasta, locations[a:b], f.write, sites_per_launch=args.sites_per_launch,
                           reads_seed=args.reads_seed, use_var_type_threshold=args.use_var_type_threshold,
                           log=lambda m: print(m, end="\r"), stats=stats, encoder_counts=counts, inflate_device=args.inflate_device,
                           first_record=first, census=flags[a:b], **(dict(sub, stage=score_stage) if sub else {}))
    for k in ("locations", "gpu", "native", "python", "no_record"):
        counts.setdefault(k, 0)
    return n


TRAIN_BAM_VCFS = ("train_tp_vcf", "train_tp_full_vcf", "train_fn_vcf", "train_fp_vcf")
TEST_BAM_VCFS = ("test_tp_vcf", "test_tp_full_vcf", "test_fn_vcf", "test_fp_vcf")


def flag(name: str) -> str:
    return "--" + name


def check_train_bam_arguments(args) -> None:
    """--train_bam and the flags that belong to it: what they need and what they refuse, before anything touches a device."""
    get = lambda k: getattr(args, k, None)   # noqa: E731
    if not get("train_bam"):
        given = [flag(k) for k in ("train_fasta",) + TRAIN_BAM_VCFS if get(k)]
        if given:
            raise SystemExit("%s belong(s) to --train_bam, which is not given (a --train_file holds its labels already)" % ", ".join(given))
        given = [flag(k) for k in TEST_BAM_VCFS if get(k)]
        if given:
            raise SystemExit("%s belong(s) to --test_bam beside --train_bam (the labelled evaluation locations); %s"
                             % (", ".join(given), "inference from --test_bam takes its locations from --sample_vcf" if args.test_bam
                                else "--test_bam is not given"))
        return
    if args.train_file:
        raise SystemExit("--train_file and --train_bam are two sources of the same records: give exactly one")
    if not get("train_fasta"):
        raise SystemExit("--train_bam needs --train_fasta (the reference)")
    if not any(get(k) for k in ("train_tp_vcf", "train_fn_vcf", "train_fp_vcf")):
        raise SystemExit("--train_bam needs its labelled locations: at least one of --train_tp_vcf (label 0), --train_fn_vcf (1), "
                         "--train_fp_vcf (2)")
    if get("train_tp_full_vcf") and not get("train_tp_vcf"):
        raise SystemExit("--train_tp_full_vcf carries the genotypes of --train_tp_vcf, which is not given")
    if args.train_loader_device != "gpu" or get("train_cache_device") != "gpu":
        raise SystemExit("--train_bam needs --train-loader-device gpu --train-cache-device gpu: the records are encoded on the GPU into "
                         "the resident record store; there is no host path and no non-resident path (convert to a --train_file with "
                         "tools/convert_bam_single_reads.py for those)")
    if bool(args.test_file) == bool(args.test_bam):
        raise SystemExit("--train_bam evaluates on exactly one of --test_file and --test_bam: %s given"
                         % ("both are" if args.test_file else "neither is"))
    if not args.test_bam:
        given = [flag(k) for k in TEST_BAM_VCFS if get(k)]
        if given:
            raise SystemExit("%s belong(s) to --test_bam, which is not given (a --test_file holds its labels already)" % ", ".join(given))
    else:
        if not args.test_fasta:
            raise SystemExit("--test_bam needs --test_fasta (the reference)")
        if get("test_tp_full_vcf") and not get("test_tp_vcf"):
            raise SystemExit("--test_tp_full_vcf carries the genotypes of --test_tp_vcf, which is not given")
        if not any(get(k) for k in ("test_tp_vcf", "test_fn_vcf", "test_fp_vcf")) and not args.sample_vcf:
            raise SystemExit("--test_bam beside --train_bam needs its locations: --test_tp_vcf / --test_fn_vcf / --test_fp_vcf, or "
                             "--sample_vcf (every location with label 2)")
    if args.record_census:
        raise SystemExit("--record-census gpu is an inference option: the resident records of --train_bam are counted when they are filled")


def check_train_loader_device_arguments(args) -> None:
    """--train-loader-device: what it refuses (the files' own properties are checked when training starts)."""
    if args.train_loader_device != "gpu":
        raise SystemExit("--train-loader-device must be gpu")
    if not args.train_file and not getattr(args, "train_bam", None):
        raise SystemExit("--train-loader-device gpu is an option of --train_file (it assembles the training and evaluation batches "
                         "on the GPU); inference from a --test_file has --loader-device gpu")


def check_train_cache_arguments(args) -> None:
    """--train-cache-device / --train-cache-bytes / --train-cache-format: what they refuse (whether the files fit is known when they
    are filled)."""
    device, budget = getattr(args, "train_cache_device", None), getattr(args, "train_cache_bytes", None)
    record_format = getattr(args, "train_cache_format", None)
    if device is None and budget is None:
        raise SystemExit("--train-cache-format is the record format of --train-cache-device gpu, which is not given")
    if device is None:
        raise SystemExit("--train-cache-bytes is the budget of --train-cache-device gpu, which is not given")
    if device != "gpu":
        raise SystemExit("--train-cache-device must be gpu")
    if args.train_loader_device != "gpu":
        raise SystemExit("--train-cache-device gpu keeps the records of --train-loader-device gpu resident: it needs that option")
    if budget is not None and budget < 0:
        raise SystemExit("--train-cache-bytes must not be negative (0: three quarters of the free device memory)")
    if record_format is not None and record_format not in ("rows", "compact"):
        raise SystemExit("--train-cache-format must be rows or compact")


def check_downsample_arguments(args) -> None:
    """--reads-dynamic-downsample-rate / -prob: what they refuse (nothing is silently ignored)."""
    rate, prob = args.reads_dynamic_downsample_rate, args.reads_dynamic_downsample_prob
    if not 0.0 <= rate < 1.0:
        raise SystemExit("--reads-dynamic-downsample-rate must lie in [0, 1): it is the mean share of a site's reads that is dropped "
                         "(%r given)" % rate)
    if not 0.0 <= prob <= 1.0:
        raise SystemExit("--reads-dynamic-downsample-prob must lie in [0, 1]: it is the share of the sites that are down-sampled "
                         "(%r given)" % prob)
    if (rate > 0) != (prob > 0):
        on, off = (("rate", "prob") if rate > 0 else ("prob", "rate"))
        raise SystemExit("--reads-dynamic-downsample-%s is given without --reads-dynamic-downsample-%s: no site would be down-sampled; "
                         "give both or neither" % (on, off))
    if rate > 0 and not args.train_file and not getattr(args, "train_bam", None):
        raise SystemExit("--reads-dynamic-downsample-rate / -prob are training options: they need --train_file or --train_bam "
                         "(evaluation and inference never down-sample)")


def check_subsample_arguments(args):
    """--subsample / --subsample-seed: (fraction, seed) or None; every refusal with its reason, before anything touches a device."""
    f, s = getattr(args, "subsample", None), getattr(args, "subsample_seed", None)
    if f is None:
        if s is not None:
            raise SystemExit("--subsample-seed %d without --subsample: the seed chooses among subsets of a fraction" % s)
        return None
    if not args.test_bam and not getattr(args, "train_bam", None):
        raise SystemExit("--subsample thins the reads of --test_bam / --train_bam, and this run reads no BAM: a --test_file or "
                         "--train_file holds pileups already encoded (give the flag to the converter that writes it)")
    if not (0.0 < f <= 1.0):
        raise SystemExit("--subsample %r: the fraction must lie in (0, 1]" % (f,))
    s = 0 if s is None else s
    if not (0 <= s < 1 << 32):
        raise SystemExit("--subsample-seed %d: the seed must lie in [0, 2^32)" % s)
    return (f, s)


def check_read_filter_arguments(args):
    """--min-mapq / --exclude-flags / --require-flags / --read-stats: (exclude, require, min_mapq) or None; every refusal with its
    reason, before anything touches a device."""
    import types
    from dl4vc_amd import read_filter

    def fail(why):
        raise SystemExit(why)

    def mask(name):
        v = getattr(args, name, None)
        if v is None or isinstance(v, int):
            return v
        try:
            return int(v, 0)
        except ValueError:
            fail("--%s %r is not a number (decimal or 0x...)" % (name.replace("_", "-"), v))

    given = types.SimpleNamespace(min_mapq=getattr(args, "min_mapq", None), exclude_flags=mask("exclude_flags"),
                                  require_flags=mask("require_flags"), read_stats=bool(getattr(args, "read_stats", False)))
    return read_filter.check(given, fail, bool(args.test_bam or getattr(args, "train_bam", None)),
                             "--test_bam / --train_bam (a --test_file or --train_file holds pileups already encoded: give the flags "
                             "to the converter that writes it)")


def bam_encoder_options(args):
    """What the BAM consumers encode with: None (their default, what call_variants.sh passes to the converter) without
    --subsample and the read filter flags, else that default with them."""
    rule = check_subsample_arguments(args)
    flt = check_read_filter_arguments(args)
    stats = bool(getattr(args, "read_stats", False))
    if rule is None and flt is None and not stats:
        return None
    from dl4vc_amd.location_round import default_encoder_options, with_read_filter, with_subsample
    return with_read_filter(with_subsample(default_encoder_options(), rule), flt, stats)


def read_filter_text(args, stage) -> str:
    from dl4vc_amd import read_filter
    flt = check_read_filter_arguments(args)
    lines = [read_filter.report_line(stage, flt) + " (the GPU encoder's records)"] if flt is not None else []
    if getattr(args, "read_stats", False):
        lines.append(read_filter.census_text(stage))
    return "\n".join(lines)


def subsample_text(args, stage) -> str:
    from dl4vc_amd.subsample import report_line
    return report_line(int(stage.get("subsample_records_seen", 0)), int(stage.get("subsample_records_kept", 0)),
                       check_subsample_arguments(args)) + " (the GPU encoder's records)"


def check_loader_device_arguments(args) -> None:
    """--loader-device: what it refuses (the file's own properties are checked when it is opened)."""
    if args.loader_device != "gpu":
        raise SystemExit("--loader-device must be gpu")
    if args.test_bam:
        raise SystemExit("--loader-device gpu is an option of --test_file (it inflates the candidate file's chunks on the GPU); "
                         "--test_bam reads no candidate file (its device option is --inflate-device gpu)")
    if args.train_file or getattr(args, "train_bam", None):
        raise SystemExit("--loader-device gpu is an inference option: training and its evaluation keep the host loaders")


def main(argv=None) -> int:
    args = parse_args(argv)
    print(args)
    if args.inflate_device not in (None, "gpu"):
        raise SystemExit("--inflate-device must be gpu")
    train_bam = getattr(args, "train_bam", None)
    if args.inflate_device and not args.test_bam and not train_bam:
        raise SystemExit("--inflate-device gpu is an option of --test_bam (the GPU pileup encoder reads the BAM); a --test_file holds "
                         "pileups already encoded")
    if args.record_census not in (None, "gpu"):
        raise SystemExit("--record-census must be gpu")
    if args.record_census and not args.test_bam:
        raise SystemExit("--record-census gpu is an option of --test_bam (it counts the locations of the candidate VCF that give a "
                         "record); the records of a --test_file are already counted")
    check_train_bam_arguments(args)
    check_subsample_arguments(args)
    check_read_filter_arguments(args)
    check_downsample_arguments(args)
    if args.loader_device is not None:
        check_loader_device_arguments(args)
    if args.train_loader_device is not None:
        check_train_loader_device_arguments(args)
    if hasattr(args, "train_cache_device") or hasattr(args, "train_cache_bytes") or hasattr(args, "train_cache_format"):
        check_train_cache_arguments(args)
    if args.test_bam and not train_bam:
        check_bam_arguments(args)
    if args.train_file or train_bam:
        return train_main(args, list(argv if argv is not None else sys.argv[1:]))
    if not args.test_bam:
        assert args.test_file[-3:] == "hdf", "Test dataset must be in HDF format"                 # main.py:84
    print("\n\nRunning in inference only mode...\n\n")
    assert args.modelload is not None, "--modelload argument is required when running in inference only mode"   # main.py:215
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.shard import parse_shard, part_path, concat_parts
    from dl4vc_amd.vcf import scored_vcf_path, start_scored_vcf

    cfg = DanConfig.from_args(args)                           # rejects unsupported model options loudly
    if args.precision not in ("fp32", "bf16x3", "bf16"):
        raise SystemExit("--precision must be fp32, bf16x3 or bf16")
    if args.conv_algo not in ("auto", "direct", "winograd"):
        raise SystemExit("--conv-algo must be auto, direct or winograd")
    import dataclasses
    cfg = dataclasses.replace(cfg, precision=("fp32", "bf16x3", "bf16").index(args.precision),
                              conv_algo=("auto", "direct", "winograd").index(args.conv_algo),
                              skip_empty_rows=not args.compute_empty_rows)
    # Data-path flags that change WHICH sites reach the VCF: honoured or refused, never silently ignored.
    if args.shuffle_test:
        # main.py:90-92: DataLoader(shuffle=True) / an unseeded np.random.permutation -- the reference's order is not
        # reproducible and call_variants.sh sorts the records afterwards (:151); the set of sites is unchanged
        raise SystemExit("--shuffle_test is not supported: the reference's shuffled order is unseeded and the pipeline sorts "
                         "the scored records anyway (call_variants.sh:151); drop the flag")
    holdout = tuple(str(c) for c in (args.test_holdout_chromosomes or ()))
    # trainer.py:513-515: the loop breaks when batch > max_test_batches, batches of --test-batch-size sites
    site_limit = (args.max_test_batches + 1) * args.test_batch_size if args.max_test_batches > 0 else 0
    shard_i, shard_n = parse_shard(args.shard)
    if args.save_vcf_records:
        assert args.save_vcf_records_file != "", "Need a valid filename for args.save_vcf_records_file to save records"
    out_base = args.save_vcf_records_file or os.path.join(os.path.dirname(args.test_bam or args.test_file), "model_test.vcf")
    out_final = scored_vcf_path(out_base)                     # <dir>/epoch1_<basename>, dl4vc/utils.py:152

    if args.gpus > 1 and not args.shard:
        # one process per GPU, contiguous shards, host-side concat
        t0 = time.time()
        procs = []
        devices = child_devices(args.gpus)
        census = bool(args.test_bam and args.record_census)
        if census:
            from dl4vc_amd.shard import remove_census
            remove_census(out_final, args.gpus)               # (a sibling never reads the census of an earlier run)
        for g in range(args.gpus):
            env = dict(os.environ, HIP_VISIBLE_DEVICES=devices[g], HSA_ENABLE_IPC_MODE_LEGACY="0")
            env.pop("CUDA_VISIBLE_DEVICES", None)             # (HIP honours both; the mask is carried in HIP_VISIBLE_DEVICES)
            if census:
                env[CENSUS_SIBLINGS] = str(args.gpus)
            cmd = [sys.executable, os.path.abspath(__file__)] + list(argv or sys.argv[1:]) + ["--shard", "%d/%d" % (g, args.gpus)]
            procs.append(subprocess.Popen(cmd, env=env))
        rcs = wait_children(procs)
        if census:
            remove_census(out_final, args.gpus)
        if any(rcs):
            for g in range(args.gpus):                        # no half-written parts left behind
                try:
                    os.remove(part_path(out_final, g))
                except OSError:
                    pass
            raise SystemExit("shard process failed: %s" % rcs)
        t_shards = time.time() - t0
        # what each shard did (its own scoring-loop clock, written beside its part file) and what the host-side concat costs: the
        # first run on a real multi-GPU node explains itself
        import json
        total = 0
        for g in range(args.gpus):
            side = part_path(out_final, g) + ".stats.json"
            try:
                with open(side) as f:
                    st = json.load(f)
                os.remove(side)
                total += st["sites"]
                print("\tshard %d/%d on device %s: %d sites, scoring loop %.2f s = %.0f sites/s (process %.2f s incl. start-up and "
                      "checkpoint load)%s" % (g, args.gpus, devices[g], st["sites"], st["loop_s"], st["sites"] / max(st["loop_s"], 1e-9),
                                              st["process_s"], census_text(st)))
            except (OSError, ValueError, KeyError):
                print("\tshard %d/%d: no statistics file" % (g, args.gpus))
        t1 = time.time()
        concat_parts(out_final, args.gpus, header_from=args.sample_vcf)
        t_cat = time.time() - t1
        print("\t%d shards: %d sites in %.2f s = %.0f sites/s whole job; host-side concat %.3f s" %
              (args.gpus, total, t_shards + t_cat, total / max(t_shards + t_cat, 1e-9), t_cat))
        print("\tTime elapsed for inference/testing {:.4f}".format(time.time() - t0))
        return 0

    if args.test_bam or args.loader_device:
        # this path shares device buffers and streams with torch: torch's HIP runtime has to be the process's only one, so it
        # is loaded before libdl4vc_dan.so brings in its own
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("%s needs a HIP device visible to torch; there is no CPU path"
                             % ("--test_bam" if args.test_bam else "--loader-device gpu"))
    from dl4vc_amd.model import DanNet, load_checkpoint
    from dl4vc_amd.inference import run_shard

    s_eval = time.time()
    print("Loading model checkpoint from {}".format(args.modelload))
    net = DanNet(cfg, device_id=0, max_batch=args.sites_per_launch).load_state_dict(load_checkpoint(args.modelload))
    if shard_n > 1:
        target = part_path(out_final, shard_i)
    else:
        target = out_final + ".records"
    t_loop = time.time()
    stats = None if os.environ.get("DL4VC_NO_THRESHOLD_STATS") else {}      # (the near-threshold count is a log line: opt out for raw rate)
    counts = {}
    loader_stage = {}
    census_stats = {}
    score_stage = {}                                          # the encoder's stages summed over the scoring calls
    if args.test_bam and args.record_census:
        n = score_bam_census(args, net, target, out_final, shard_i, shard_n, holdout, site_limit, stats, counts, census_stats, score_stage)
    elif args.test_bam:
        # the encoder options are what call_variants.sh passes to the converter (score_bam's default)
        from dl4vc_amd.inference import score_bam
        from dl4vc_amd.pileup_encoder import locations_from_vcf
        locations = locations_from_vcf(args.sample_vcf, label=2)
        with open(target, "w") as f:
            n = score_bam(net, args.test_bam, args.test_fasta, locations, f.write, sites_per_launch=args.sites_per_launch,
                          reads_seed=args.reads_seed, use_var_type_threshold=args.use_var_type_threshold, site_limit=site_limit,
                          log=lambda m: print(m, end="\r"), stats=stats, encoder_counts=counts, inflate_device=args.inflate_device,
                          encoder_options=bam_encoder_options(args), stage=score_stage)
    else:
        extra = {"loader_device": "gpu", "loader_stats": loader_stage} if args.loader_device else {}
        try:
            n = run_shard(net, args.test_file, target, shard_i, shard_n, sites_per_launch=args.sites_per_launch,
                          reads_seed=args.reads_seed, use_var_type_threshold=args.use_var_type_threshold,
                          holdout_chromosomes=holdout, site_limit=site_limit, log=lambda m: print(m, end="\r"), stats=stats, **extra)
        except (ValueError, RuntimeError) as e:
            if not args.loader_device:
                raise
            raise SystemExit("--loader-device gpu: %s" % e)   # (a refused file or a damaged chunk: the reason, not a traceback)
    t_loop = time.time() - t_loop - census_stats.get("census_s", 0.0) - census_stats.get("census_wait_s", 0.0)
    net.close()
    if getattr(args, "subsample", None) is not None:
        print("\n" + subsample_text(args, score_stage))
    text = read_filter_text(args, score_stage)
    if text:
        print("\n" + text)
    if census_stats:
        print("\nrecord census: %s" % census_text(census_stats).lstrip("; "))
    if args.test_bam:
        print("\npileup encoder: %d locations: %d on the GPU, %d by pe_encode, %d by the Python builder, %d without a record"
              % tuple(counts[k] for k in ("locations", "gpu", "native", "python", "no_record")))
    if loader_stage:
        print("\ndevice loader: %s" % ", ".join("%s %s" % (k, ("%.1f" % v) if k.endswith("_ms") else int(v)) for k, v in loader_stage.items()))
    if stats is not None:
        print("\n%d of %d sites lie within 1e-4 of a genotype threshold of the published pipeline (format_vcf flags of "
              "call_variants.sh:154-160; main.py has no threshold flags of its own -- tools/format_vcf.py takes them later): only "
              "there could a call differ from another correct fp32 evaluation of the same scores"
              % (stats.get("near_threshold", 0), stats.get("sites", 0)))
    print("\nscoring loop (%s + assembly + forward + VCF text): %d sites in %.2f s = %.0f sites/s"
          % ("BAM fetch + pileup encoder" if args.test_bam else "HDF5 raw chunks + device inflate" if args.loader_device else "HDF5 read",
             n, t_loop, n / max(t_loop, 1e-9)))
    if shard_n == 1:
        if args.sample_vcf:
            start_scored_vcf(args.sample_vcf, out_base)
        else:
            open(out_final, "w").close()
        with open(out_final, "a") as out, open(target) as src:
            out.write(src.read())
        os.remove(target)
    if shard_n > 1:
        import json
        with open(target + ".stats.json", "w") as f:
            json.dump(dict({"sites": int(n), "loop_s": t_loop, "process_s": time.time() - s_eval, "shard": shard_i, "of": shard_n},
                           **census_stats), f)
    print("\nscored %d sites -> %s" % (n, out_final if shard_n == 1 else target))
    print("\tTime elapsed for inference/testing {:.4f}".format(time.time() - s_eval))
    return 0


if __name__ == "__main__":
    sys.exit(main())
