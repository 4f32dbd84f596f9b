/*
 * main_gpu.c — pcktbatch-gpu: the reference's program entry (src/main.c)
 * with the packet build on MI355X.
 *
 * Same two-pass command line as main.c:23-94 (opterr = 0; common options,
 * then optind = 0 and the AF_XDP options of cmd_line.c plus this build's GPU
 * options), the first-sequence override (-z, README.md:101-151), sequences
 * run in order through seq_send(), shutdown_prog() on exit or SIGINT/SIGTERM.
 * The JSON config (-c, default /etc/pcktbatch/conf.json) is read first and the
 * -z overrides are applied to its first sequence afterwards, as main.c:90-103
 * does with PB-Common's parse_config() / parse_cli() (host/config_json.c).
 * Frames go through a TX ring: an AF_XDP socket per thread with --tx xsk,
 * otherwise the in-memory ring of host/xsk_ring.c, whose consumer writes a pcap
 * file with --pcap (or only counts).
 */
#include <arpa/inet.h>
#include <getopt.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cmd_line.h"
#include "config_json.h"
#include "pcap_dump.h"
#include "sequence_gpu.h"

typedef struct cmd_line
{
    const char *config;
    int cli, list, verbose, help;
} cmd_line_t;

static pb_config_t *cfg;
/* --pcapdump FILE [--pcapt0 NS] (pcap_dump.h): this file's own options, kept out of
 * struct cmd_line_af_xdp, whose layout other programs bind */
static const char *pcapdump_path;
static int pcapt0_set;
static uint64_t pcapt0_ns;
/* --encap vlan:VID[:PCP] | vxlan:VNI:SRCIP:DSTIP[:DPORT], once: handed to the driver with pb_set_encap */
static const char *encap_spec;
static int encap_twice;
/* --fragment MTU[:ignoredf], once: handed to the driver with pb_set_fragment */
static const char *fragment_spec;
static int fragment_twice;
/* --segment MSS[:fixedid], once: handed to the driver with pb_set_segment */
static const char *segment_spec;
static int segment_twice;
/* --stamp head[:OFF] | tail[:OFF], once: handed to the driver with pb_set_stamp */
static const char *stamp_spec;
static int stamp_twice;
/* --xlat6 SRC6/96[,DST6/96][:hashflow], once: handed to the driver with pb_set_xlat */
static const char *xlat_spec;
static int xlat_twice;
/* --verifywire: handed to the driver with pb_set_verify_wire */
static int verify_wire;

static void sign_hdl(int sig)
{
    (void)sig;
    pb_request_stop();
}

enum
{
    O_INTERFACE = 256, O_BLOCK, O_TRACK, O_MAXPCKTS, O_MAXBYTES, O_PPS, O_BPS, O_DELAY, O_THREADS, O_L4CSUM, O_SMAC,
    O_DMAC, O_MINTTL, O_MAXTTL, O_MINID, O_MAXID, O_SIP, O_DIP, O_PROTOCOL, O_TOS, O_L3CSUM, O_USPORT, O_UDPORT,
    O_TSPORT, O_TDPORT, O_SYN, O_ACK, O_PSH, O_RST, O_FIN, O_URG, O_ECE, O_CWR, O_PMIN, O_PMAX, O_PSTATIC, O_PEXACT,
    O_PFILE, O_PSTRING, O_TIME, O_SECOND_PASS, O_PCAPDUMP, O_PCAPT0, O_ENCAP, O_FRAGMENT, O_STAMP,
    O_XLAT6, O_VERIFYWIRE, O_SEGMENT,
};

static const struct option common_opts[] = {
    {"cfg", required_argument, NULL, 'c'},   {"list", no_argument, NULL, 'l'},
    {"verbose", no_argument, NULL, 'v'},     {"help", no_argument, NULL, 'h'},
    {"cli", no_argument, NULL, 'z'},         {"interface", required_argument, NULL, O_INTERFACE},
    {"block", required_argument, NULL, O_BLOCK}, {"track", required_argument, NULL, O_TRACK},
    {"maxpckts", required_argument, NULL, O_MAXPCKTS}, {"maxbytes", required_argument, NULL, O_MAXBYTES},
    {"pps", required_argument, NULL, O_PPS}, {"bps", required_argument, NULL, O_BPS},
    {"delay", required_argument, NULL, O_DELAY}, {"threads", required_argument, NULL, O_THREADS},
    {"l4csum", required_argument, NULL, O_L4CSUM}, {"smac", required_argument, NULL, O_SMAC},
    {"dmac", required_argument, NULL, O_DMAC}, {"minttl", required_argument, NULL, O_MINTTL},
    {"maxttl", required_argument, NULL, O_MAXTTL}, {"minid", required_argument, NULL, O_MINID},
    {"maxid", required_argument, NULL, O_MAXID}, {"sip", required_argument, NULL, O_SIP},
    {"dip", required_argument, NULL, O_DIP}, {"protocol", required_argument, NULL, O_PROTOCOL},
    {"tos", required_argument, NULL, O_TOS}, {"l3csum", required_argument, NULL, O_L3CSUM},
    {"usport", required_argument, NULL, O_USPORT}, {"udport", required_argument, NULL, O_UDPORT},
    {"tsport", required_argument, NULL, O_TSPORT}, {"tdport", required_argument, NULL, O_TDPORT},
    {"syn", required_argument, NULL, O_SYN}, {"ack", required_argument, NULL, O_ACK},
    {"psh", required_argument, NULL, O_PSH}, {"rst", required_argument, NULL, O_RST},
    {"fin", required_argument, NULL, O_FIN}, {"urg", required_argument, NULL, O_URG},
    {"ece", required_argument, NULL, O_ECE}, {"cwr", required_argument, NULL, O_CWR},
    {"pmin", required_argument, NULL, O_PMIN}, {"pmax", required_argument, NULL, O_PMAX},
    {"pstatic", required_argument, NULL, O_PSTATIC}, {"pexact", required_argument, NULL, O_PEXACT},
    {"pfile", required_argument, NULL, O_PFILE}, {"pstring", required_argument, NULL, O_PSTRING},
    {"time", required_argument, NULL, O_TIME},
    /* parsed in the second pass (cmd_line.c); listed here so that GNU getopt's
     * argument permutation never separates them from their values */
    {"queue", required_argument, NULL, O_SECOND_PASS}, {"batchsize", required_argument, NULL, O_SECOND_PASS},
    {"nowakeup", no_argument, NULL, O_SECOND_PASS}, {"sharedumem", no_argument, NULL, O_SECOND_PASS},
    {"skb", no_argument, NULL, O_SECOND_PASS}, {"zerocopy", no_argument, NULL, O_SECOND_PASS},
    {"copy", no_argument, NULL, O_SECOND_PASS}, {"gpus", required_argument, NULL, O_SECOND_PASS},
    {"gpu", required_argument, NULL, O_SECOND_PASS}, {"gpubatch", required_argument, NULL, O_SECOND_PASS},
    {"seed", required_argument, NULL, O_SECOND_PASS}, {"literal", no_argument, NULL, O_SECOND_PASS},
    {"singlefold", no_argument, NULL, O_SECOND_PASS}, {"pcap", required_argument, NULL, O_SECOND_PASS},
    {"tx", required_argument, NULL, O_SECOND_PASS}, {"veryrandom", no_argument, NULL, O_SECOND_PASS},
    {"umemframes", required_argument, NULL, O_SECOND_PASS}, {"umemslot", required_argument, NULL, O_SECOND_PASS},
    {"verify", no_argument, NULL, O_SECOND_PASS},
    {"pcapdump", required_argument, NULL, O_PCAPDUMP}, {"pcapt0", required_argument, NULL, O_PCAPT0},
    {"encap", required_argument, NULL, O_ENCAP}, {"fragment", required_argument, NULL, O_FRAGMENT},
    {"stamp", required_argument, NULL, O_STAMP}, {"xlat6", required_argument, NULL, O_XLAT6},
    {"verifywire", no_argument, NULL, O_VERIFYWIRE}, {"segment", required_argument, NULL, O_SEGMENT},
    {NULL, 0, NULL, 0},
};

/* defaults of one sequence (README.md:216-575; PB-Common clear_sequence) */
static void clear_sequence(pb_config_t *c, int i)
{
    pb_sequence_t *s = &c->seq[i];
    memset(s, 0, sizeof *s);
    s->block = 1;
    s->delay = 1000000;
    s->l4_csum = 1;
    s->ip.csum = 1;
    s->ip.min_ttl = 64;
    s->ip.max_ttl = 64;
    s->ip.max_id = 64000;
}

/* first pass: common options and the -z overrides of sequence 0 */
static void parse_common(int argc, char **argv, cmd_line_t *cmd, pb_sequence_t *s, const char **iface)
{
    int o;
    while ((o = getopt_long(argc, argv, "c:lvhz", common_opts, NULL)) != -1)
    {
        const char *a = optarg;
        switch (o)
        {
        case 'c': cmd->config = a; break;
        case 'l': cmd->list = 1; break;
        case 'v': cmd->verbose = 1; break;
        case 'h': cmd->help = 1; break;
        case 'z': cmd->cli = 1; break;
        case O_INTERFACE: *iface = a; s->interface = a; break;
        case O_BLOCK: s->block = (uint8_t)atoi(a); break;
        case O_TRACK: s->track = (uint8_t)atoi(a); break;
        case O_MAXPCKTS: s->max_pckts = strtoull(a, NULL, 10); break;
        case O_MAXBYTES: s->max_bytes = strtoull(a, NULL, 10); break;
        case O_PPS: s->pps = strtoull(a, NULL, 10); break;
        case O_BPS: s->bps = strtoull(a, NULL, 10); break;
        case O_DELAY: s->delay = strtoull(a, NULL, 10); break;
        case O_THREADS: s->threads = (uint16_t)atoi(a); break;
        case O_L4CSUM: s->l4_csum = (uint8_t)atoi(a); break;
        case O_SMAC: s->eth.src_mac = a; break;
        case O_DMAC: s->eth.dst_mac = a; break;
        case O_MINTTL: s->ip.min_ttl = (uint8_t)atoi(a); break;
        case O_MAXTTL: s->ip.max_ttl = (uint8_t)atoi(a); break;
        case O_MINID: s->ip.min_id = (uint16_t)atoi(a); break;
        case O_MAXID: s->ip.max_id = (uint16_t)atoi(a); break;
        case O_SIP: /* "one range is supported in CIDR format" (README.md:132) */
            if (strchr(a, '/'))
            {
                s->ip.ranges[0] = a;
                s->ip.range_count = 1;
                s->ip.src_ip = NULL;
            }
            else
            {
                s->ip.src_ip = a;
            }
            break;
        case O_DIP: s->ip.dst_ip = a; break;
        case O_PROTOCOL: s->ip.protocol = a; break;
        case O_TOS: s->ip.tos = (uint8_t)atoi(a); break;
        case O_L3CSUM: s->ip.csum = (uint8_t)atoi(a); break;
        case O_USPORT: s->udp.src_port = (uint16_t)atoi(a); break;
        case O_UDPORT: s->udp.dst_port = (uint16_t)atoi(a); break;
        case O_TSPORT: s->tcp.src_port = (uint16_t)atoi(a); break;
        case O_TDPORT: s->tcp.dst_port = (uint16_t)atoi(a); break;
        case O_SYN: s->tcp.syn = (uint8_t)atoi(a); break;
        case O_ACK: s->tcp.ack = (uint8_t)atoi(a); break;
        case O_PSH: s->tcp.psh = (uint8_t)atoi(a); break;
        case O_RST: s->tcp.rst = (uint8_t)atoi(a); break;
        case O_FIN: s->tcp.fin = (uint8_t)atoi(a); break;
        case O_URG: s->tcp.urg = (uint8_t)atoi(a); break;
        case O_ECE: s->tcp.ece = (uint8_t)atoi(a); break;
        case O_CWR: s->tcp.cwr = (uint8_t)atoi(a); break;
        case O_PMIN: s->pls[0].min_len = (uint16_t)atoi(a); s->pl_cnt = 1; break;
        case O_PMAX: s->pls[0].max_len = (uint16_t)atoi(a); s->pl_cnt = 1; break;
        case O_PSTATIC: s->pls[0].is_static = (uint8_t)atoi(a); s->pl_cnt = 1; break;
        case O_PEXACT: s->pls[0].exact = a; s->pl_cnt = 1; break;
        case O_PFILE: s->pls[0].is_file = (uint8_t)atoi(a); s->pl_cnt = 1; break;
        case O_PSTRING: s->pls[0].is_string = (uint8_t)atoi(a); s->pl_cnt = 1; break;
        case O_TIME: s->time = strtoull(a, NULL, 10); break;
        case O_PCAPDUMP: pcapdump_path = a; break;
        case O_PCAPT0: pcapt0_ns = strtoull(a, NULL, 10); pcapt0_set = 1; break;
        case O_ENCAP: /* the -z pass reads the same argument again */
            if (encap_spec && encap_spec != a)
                encap_twice = 1;
            encap_spec = a;
            break;
        case O_FRAGMENT:
            if (fragment_spec && fragment_spec != a)
                fragment_twice = 1;
            fragment_spec = a;
            break;
        case O_STAMP:
            if (stamp_spec && stamp_spec != a)
                stamp_twice = 1;
            stamp_spec = a;
            break;
        case O_XLAT6:
            if (xlat_spec && xlat_spec != a)
                xlat_twice = 1;
            xlat_spec = a;
            break;
        case O_VERIFYWIRE: verify_wire = 1; break;
        case O_SEGMENT:
            if (segment_spec && segment_spec != a)
                segment_twice = 1;
            segment_spec = a;
            break;
        default: break;
        }
    }
}

/* a decimal number in [0, max] filling the whole field */
static int field_u32(const char *s, uint32_t max, uint32_t *out)
{
    if (s == NULL || *s < '0' || *s > '9')
        return -1;
    char *end = NULL;
    const unsigned long long v = strtoull(s, &end, 10);
    if (*end != '\0' || v > max)
        return -1;
    *out = (uint32_t)v;
    return 0;
}

/* --encap's argument -> the options the driver completes with each sequence's MACs; -1 and a
 * message in `why` for a malformed one */
static int parse_encap(const char *spec, pbgpu_encap_opts *o, const char **why)
{
    char buf[128];
    char *f[6] = {NULL};
    int nf = 0;
    memset(o, 0, sizeof *o);
    if (strlen(spec) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    strcpy(buf, spec);
    for (char *p = buf; nf < 6; ++nf)
    {
        f[nf] = p;
        p = strchr(p, ':');
        if (p == NULL)
        {
            ++nf;
            break;
        }
        *p++ = '\0';
    }
    uint32_t v = 0;
    if (strcmp(f[0], "vlan") == 0)
    {
        o->mode = PBGPU_ENCAP_VLAN;
        if (nf < 2 || nf > 3)
        {
            *why = "expected vlan:VID[:PCP]";
            return -1;
        }
        if (field_u32(f[1], 4095, &v) != 0)
        {
            *why = "VID is 0-4095";
            return -1;
        }
        o->tci = (uint16_t)v;
        if (nf == 3)
        {
            if (field_u32(f[2], 7, &v) != 0)
            {
                *why = "PCP is 0-7";
                return -1;
            }
            o->tci |= (uint16_t)(v << 13);
        }
        return 0;
    }
    if (strcmp(f[0], "vxlan") == 0)
    {
        o->mode = PBGPU_ENCAP_VXLAN;
        if (nf < 4 || nf > 5)
        {
            *why = "expected vxlan:VNI:SRCIP:DSTIP[:DPORT]";
            return -1;
        }
        if (field_u32(f[1], (1u << 24) - 1, &v) != 0)
        {
            *why = "VNI is 0-16777215";
            return -1;
        }
        o->vni = v;
        if (inet_pton(AF_INET, f[2], o->src_ip) != 1 || inet_pton(AF_INET, f[3], o->dst_ip) != 1)
        {
            *why = "SRCIP and DSTIP are dotted IPv4 addresses";
            return -1;
        }
        if (nf == 5)
        {
            if (field_u32(f[4], 65535, &v) != 0 || v == 0)
            {
                *why = "DPORT is 1-65535";
                return -1;
            }
            o->dst_port = (uint16_t)v;
        }
        return 0;
    }
    *why = "expected vlan:... or vxlan:...";
    return -1;
}

/* --fragment's argument MTU[:ignoredf] -> the options; -1 and a message in `why` for a malformed one */
static int parse_fragment(const char *spec, pbgpu_frag_opts *o, const char **why)
{
    char buf[32];
    memset(o, 0, sizeof *o);
    if (strlen(spec) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    strcpy(buf, spec);
    char *opt = strchr(buf, ':');
    if (opt)
        *opt++ = '\0';
    uint32_t v = 0;
    if (field_u32(buf, 65535, &v) != 0 || v < 68)
    {
        *why = "MTU is 68-65535";
        return -1;
    }
    o->mtu = v;
    if (opt)
    {
        if (strcmp(opt, "ignoredf") != 0)
        {
            *why = "expected MTU[:ignoredf]";
            return -1;
        }
        o->flags = PBGPU_FRAG_IGNORE_DF;
    }
    return 0;
}

/* --segment's argument MSS[:fixedid] -> the options; -1 and a message in `why` for a malformed one */
static int parse_segment(const char *spec, pbgpu_seg_opts *o, const char **why)
{
    char buf[32];
    memset(o, 0, sizeof *o);
    if (strlen(spec) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    strcpy(buf, spec);
    char *opt = strchr(buf, ':');
    if (opt)
        *opt++ = '\0';
    uint32_t v = 0;
    if (field_u32(buf, 65535, &v) != 0 || v < 8)
    {
        *why = "MSS is 8-65535";
        return -1;
    }
    o->mss = v;
    if (opt)
    {
        if (strcmp(opt, "fixedid") != 0)
        {
            *why = "expected MSS[:fixedid]";
            return -1;
        }
        o->flags = PBGPU_SEG_FIXED_ID;
    }
    return 0;
}

/* --stamp's argument head[:OFF] | tail[:OFF] -> the offset and flags; -1 and a message in `why` for a
 * malformed one */
static int parse_stamp(const char *spec, pbgpu_stamp_opts *o, const char **why)
{
    char buf[32];
    memset(o, 0, sizeof *o);
    if (strlen(spec) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    strcpy(buf, spec);
    char *off = strchr(buf, ':');
    if (off)
        *off++ = '\0';
    if (strcmp(buf, "tail") == 0)
        o->flags = PBGPU_STAMP_TAIL;
    else if (strcmp(buf, "head") != 0)
    {
        *why = "expected head[:OFF] or tail[:OFF]";
        return -1;
    }
    if (off && field_u32(off, 65535, &o->offset) != 0)
    {
        *why = "OFF is 0-65535 bytes";
        return -1;
    }
    return 0;
}

/* one SRC6/96 of --xlat6 -> its 12 prefix bytes */
static int parse_prefix96(const char *s, uint8_t out[12], const char **why)
{
    char buf[64];
    uint8_t a[16];
    const char *slash = strchr(s, '/');
    if (slash == NULL || strcmp(slash, "/96") != 0)
    {
        *why = "a prefix is written ADDR6/96: only /96 prefixes (RFC 6052) are translated";
        return -1;
    }
    if ((size_t)(slash - s) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    memcpy(buf, s, (size_t)(slash - s));
    buf[slash - s] = '\0';
    if (inet_pton(AF_INET6, buf, a) != 1)
    {
        *why = "not an IPv6 address";
        return -1;
    }
    if (a[12] | a[13] | a[14] | a[15])
    {
        *why = "address bits set beyond the /96 prefix";
        return -1;
    }
    memcpy(out, a, 12);
    return 0;
}

/* --xlat6's argument SRC6/96[,DST6/96][:hashflow] -> the options; -1 and a message in `why` for a
 * malformed one.  The suffix follows "/96", so its colon is none of an address's. */
static int parse_xlat(const char *spec, pbgpu_xlat_opts *o, const char **why)
{
    char buf[160];
    memset(o, 0, sizeof *o);
    if (strlen(spec) >= sizeof buf)
    {
        *why = "too long";
        return -1;
    }
    strcpy(buf, spec);
    char *sfx = strstr(buf, "/96:");
    if (sfx)
    {
        char *last;
        while ((last = strstr(sfx + 1, "/96:")) != NULL) /* the suffix follows the last prefix */
            sfx = last;
        sfx[3] = '\0';
        if (strcmp(sfx + 4, "hashflow") != 0)
        {
            *why = "expected SRC6/96[,DST6/96][:hashflow]";
            return -1;
        }
        o->flags = PBGPU_XLAT_HASH_FLOW;
    }
    char *second = strchr(buf, ',');
    if (second)
        *second++ = '\0';
    if (parse_prefix96(buf, o->src_prefix, why) != 0)
        return -1;
    if (second == NULL)
        memcpy(o->dst_prefix, o->src_prefix, 12);
    else if (parse_prefix96(second, o->dst_prefix, why) != 0)
        return -1;
    return 0;
}

static void print_cmd_help(void)
{
    fprintf(stdout, "Usage: pcktbatch-gpu -c <configfile> | -z [overrides] [-v -l -h] [AF_XDP/GPU options]\n\n"
                    "-c --cfg => Path to the config file (default /etc/pcktbatch/conf.json).\n"
                    "-l --list => Print basic information about sequences.\n"
                    "-v --verbose => Provide verbose output.\n"
                    "-h --help => Print out help menu and exit program.\n"
                    "-z --cli => Enables the first sequence/packet override (README.md first-sequence options).\n\n"
                    "AF_XDP: --queue --nowakeup --sharedumem --batchsize --skb --zerocopy --copy\n"
                    "GPU: --gpus N --gpu I --gpubatch K --seed S --veryrandom --literal --singlefold --pcap FILE --tx xsk "
                    "--umemframes N --umemslot S --verify --pcapdump FILE --pcapt0 NS --encap SPEC --fragment MTU[:ignoredf] "
                    "--stamp head[:OFF]|tail[:OFF] --xlat6 SRC6/96[,DST6/96][:hashflow] --verifywire --segment MSS[:fixedid]\n"
                    "--verify => Check every built batch's checksums and lengths on the GPU as it is built (and stamped): "
                    "Ethernet + IPv4 without options. Of a repacked batch it sees the IPv4 checksum and length of "
                    "fragments and of a VXLAN outer header, nothing of a VLAN or IPv6 frame.\n"
                    "--verifywire => Check every batch on the GPU as it leaves, after the last repack: VLAN tags, IPv4 "
                    "or IPv6, a VXLAN inner frame, fragments and UDP without a checksum are told from the frames' own "
                    "bytes. One more line at the end; a bad frame stops the sequence as --verify's does. May be given "
                    "beside --verify.\n"
                    "--pcapdump FILE => Write the sequences' frames (--maxpckts each) to FILE as a pcap capture packed "
                    "on the GPU; nothing is sent. Timestamps: --pcapt0 NS (ns since the epoch, default now) plus "
                    "1/pps per frame.\n"
                    "--encap vlan:VID[:PCP] | vxlan:VNI:SRCIP:DSTIP[:DPORT] => Encapsulate every frame on the GPU before "
                    "it is sent or dumped: an 802.1Q tag, or a VXLAN outer header (the sequence's MACs, TTL 64, source "
                    "port hashed from the inner frame, DPORT 4789 by default).\n"
                    "--fragment MTU[:ignoredf] => Split every built IPv4 packet longer than MTU (68-65535) into fragments "
                    "on the GPU before it is verified again, encapsulated, sent or dumped; packets with DF set are left "
                    "whole unless :ignoredf is given. --maxpckts counts built packets, the byte limits what is sent.\n"
                    "--stamp head[:OFF] | tail[:OFF] => Write BE64(frame index) and BE64(T ns) into every built ICMP / TCP / "
                    "UDP frame on the GPU, OFF bytes into its L4 payload (tail: its last 16 bytes, OFF bytes further "
                    "in), before it is verified, fragmented, encapsulated, sent or dumped; the L4 checksum is updated "
                    "unless l4csum is 0. T = t0 + index / pps: t0 is --pcapt0 NS (default now), and T is the scheduled "
                    "time, not the wire time. A frame without room stays as it is. scripts/stamp_read.py reads a "
                    "capture back.\n"
                    "--xlat6 SRC6/96[,DST6/96][:hashflow] => Translate every built frame to IPv6 on the GPU (RFC 7915, "
                    "stateless) after it is stamped and verified and before it is encapsulated, sent or dumped: the IPv4 "
                    "addresses go behind the /96 prefixes (RFC 6052; one prefix serves both), TOS and TTL carry over, the "
                    "TCP / UDP / ICMP echo checksums are updated. :hashflow hashes the flow label from addresses and "
                    "ports (default 0). Not with --fragment, nor with a UDP sequence whose l4csum is 0.\n"
                    "--segment MSS[:fixedid] => Cut every built TCP or UDP frame with more than MSS (8-65535) payload bytes "
                    "into segments of MSS bytes on the GPU, as TSO and UDP_SEGMENT do: each with its own IPv4 length, ID "
                    "(ID + i; :fixedid keeps the packet's) and checksum, its own TCP sequence number and flags or UDP "
                    "length, and an L4 checksum of its own unless l4csum is 0. After --stamp and --verify, before the "
                    "batch is verified again, fragmented, translated, encapsulated, sent or dumped. --maxpckts counts "
                    "built packets, the byte limits what is sent.\n");
}

int main(int argc, char **argv)
{
    opterr = 0; /* main.c:26 */
    cmd_line_t cmd = {0};
    cfg = (pb_config_t *)calloc(1, sizeof *cfg);
    if (cfg == NULL)
        return EXIT_FAILURE;
    for (int i = 0; i < PB_MAX_SEQUENCES; ++i)
        clear_sequence(cfg, i);
    /* getopt permutes argv (the AF_XDP pass moves the values of options it does not
     * know); the -z overrides are re-read later from this untouched copy */
    char **argv_cli = (char **)malloc(((size_t)argc + 1) * sizeof *argv_cli);
    if (argv_cli == NULL)
        return EXIT_FAILURE;
    memcpy(argv_cli, argv, ((size_t)argc + 1) * sizeof *argv_cli);
    const char *iface = NULL;
    {
        /* first pass for the common flags only (main.c:30); the -z overrides are
         * applied after the config file */
        pb_sequence_t scratch;
        memset(&scratch, 0, sizeof scratch);
        parse_common(argc, argv, &cmd, &scratch, &iface);
    }
    if (cmd.help)
    {
        print_cmd_help();
        return EXIT_SUCCESS;
    }
    if (encap_spec) /* refused before anything else is set up */
    {
        pbgpu_encap_opts eo;
        const char *why = NULL;
        if (encap_twice)
        {
            fprintf(stderr, "--encap given more than once: one encapsulation per run.\n");
            return EXIT_FAILURE;
        }
        if (parse_encap(encap_spec, &eo, &why) != 0)
        {
            fprintf(stderr, "--encap %s: %s.\n", encap_spec, why);
            return EXIT_FAILURE;
        }
        pb_set_encap(&eo);
    }
    if (fragment_spec)
    {
        pbgpu_frag_opts fo;
        const char *why = NULL;
        if (fragment_twice)
        {
            fprintf(stderr, "--fragment given more than once: one MTU per run.\n");
            return EXIT_FAILURE;
        }
        if (parse_fragment(fragment_spec, &fo, &why) != 0)
        {
            fprintf(stderr, "--fragment %s: %s.\n", fragment_spec, why);
            return EXIT_FAILURE;
        }
        pb_set_fragment(&fo);
    }
    if (segment_spec)
    {
        pbgpu_seg_opts go;
        const char *why = NULL;
        if (segment_twice)
        {
            fprintf(stderr, "--segment given more than once: one MSS per run.\n");
            return EXIT_FAILURE;
        }
        if (parse_segment(segment_spec, &go, &why) != 0)
        {
            fprintf(stderr, "--segment %s: %s.\n", segment_spec, why);
            return EXIT_FAILURE;
        }
        pb_set_segment(&go);
    }
    if (stamp_spec)
    {
        pbgpu_stamp_opts so;
        const char *why = NULL;
        if (stamp_twice)
        {
            fprintf(stderr, "--stamp given more than once: one stamp per run.\n");
            return EXIT_FAILURE;
        }
        if (parse_stamp(stamp_spec, &so, &why) != 0)
        {
            fprintf(stderr, "--stamp %s: %s.\n", stamp_spec, why);
            return EXIT_FAILURE;
        }
        so.t0_ns = pcapt0_ns; /* --pcapt0 counts without --pcapdump too */
        pb_set_stamp(&so, pcapt0_set);
    }
    if (xlat_spec)
    {
        pbgpu_xlat_opts xo;
        const char *why = NULL;
        if (xlat_twice)
        {
            fprintf(stderr, "--xlat6 given more than once: one translation per run.\n");
            return EXIT_FAILURE;
        }
        if (parse_xlat(xlat_spec, &xo, &why) != 0)
        {
            fprintf(stderr, "--xlat6 %s: %s.\n", xlat_spec, why);
            return EXIT_FAILURE;
        }
        if (fragment_spec)
        {
            fprintf(stderr, "--xlat6 does not combine with --fragment: IPv6 frames are not fragmented here.\n");
            return EXIT_FAILURE;
        }
        pb_set_xlat(&xo);
    }
    pb_set_verify_wire(verify_wire);
    struct cmd_line_af_xdp cmd_af_xdp = {0};
    cmd_line_af_xdp_defaults(&cmd_af_xdp);
    optind = 0; /* main.c:45 */
    parse_cmd_line_af_xdp(&cmd_af_xdp, argc, argv);
    pb_set_verbose(cmd.verbose);
    if (pb_af_xdp_setup(&cmd_af_xdp, cmd.verbose) != 0) /* setup_af_xdp_variables (main.c:49) */
        return EXIT_FAILURE;
    /* the seed stream's base: --seed, else drawn from CLOCK_BOOTTIME (or getrandom with
     * --veryrandom) the way the reference seeds every iteration (sequence.c:434-441) */
    pb_resolve_seed(&cmd_af_xdp);

    if (cmd.config == NULL) /* main.c:51-61 */
    {
        cmd.config = "/etc/pcktbatch/conf.json";
        if (cmd.verbose)
            fprintf(stdout, "No config specified. Using default: %s.\n", cmd.config);
    }
    int seq_cnt = 0;
    if (cmd.cli)
        fprintf(stdout, "Using command line...\n");
    const int prc = pb_parse_config(cmd.config, cfg, &seq_cnt, !cmd.cli); /* main.c:94 */
    if (prc != 0 && !cmd.cli)
        return EXIT_FAILURE;
    if (cmd.cli) /* parse_cli(): the overrides of the first sequence (main.c:96-103) */
    {
        optind = 0;
        iface = NULL;
        parse_common(argc, argv_cli, &cmd, &cfg->seq[0], &iface);
        if (iface)
            cfg->interface = iface;
        if (seq_cnt < 1)
            seq_cnt = 1;
    }
    if (cmd.list)
    {
        fprintf(stdout, "AF_XDP: queue_set=%u queue=%d nowakeup=%u sharedumem=%u batchsize=%u skb=%u zerocopy=%u copy=%u\n",
                cmd_af_xdp.queue_set, cmd_af_xdp.queue, cmd_af_xdp.no_wake_up, cmd_af_xdp.shared_umem,
                cmd_af_xdp.batch_size, cmd_af_xdp.skb_mode, cmd_af_xdp.zero_copy, cmd_af_xdp.copy);
        fprintf(stdout,
                "GPU: gpus=%d gpu=%d gpubatch=%llu seed=%llu literal=%d singlefold=%d pcap=%s tx=%s umemframes=%u "
                "umemslot=%u\n",
                cmd_af_xdp.gpus, cmd_af_xdp.gpu_first, (unsigned long long)cmd_af_xdp.gpu_batch,
                (unsigned long long)cmd_af_xdp.seed_base, cmd_af_xdp.literal_payload, cmd_af_xdp.single_fold,
                cmd_af_xdp.pcap ? cmd_af_xdp.pcap : "(none)", cmd_af_xdp.tx ? cmd_af_xdp.tx : "ring",
                cmd_af_xdp.umem_frames, cmd_af_xdp.umem_slot ? cmd_af_xdp.umem_slot : 4096u);
        if (pb_get_xlat())
        {
            const pbgpu_xlat_opts *xo = pb_get_xlat();
            uint8_t a[16] = {0};
            char s6[INET6_ADDRSTRLEN], d6[INET6_ADDRSTRLEN];
            memcpy(a, xo->src_prefix, 12);
            inet_ntop(AF_INET6, a, s6, sizeof s6);
            memcpy(a, xo->dst_prefix, 12);
            inet_ntop(AF_INET6, a, d6, sizeof d6);
            fprintf(stdout, "XLAT6: src=%s/96 dst=%s/96 hashflow=%u\n", s6, d6, xo->flags & PBGPU_XLAT_HASH_FLOW);
        }
        if (pb_get_verify_wire())
            fprintf(stdout, "VERIFYWIRE: on\n");
        for (int i = 0; i < seq_cnt; ++i)
            fprintf(stdout, "Sequence #%d: %s -> %s proto %s, %u payload(s)\n", i + 1,
                    cfg->seq[i].ip.src_ip ? cfg->seq[i].ip.src_ip
                                          : (cfg->seq[i].ip.range_count ? cfg->seq[i].ip.ranges[0] : "127.0.0.1"),
                    cfg->seq[i].ip.dst_ip ? cfg->seq[i].ip.dst_ip : "(none)",
                    cfg->seq[i].ip.protocol ? cfg->seq[i].ip.protocol : "udp", cfg->seq[i].pl_cnt);
        return EXIT_SUCCESS;
    }
    fprintf(stdout, "Seed base => 0x%016llx (%s; replay with --seed 0x%llx).\n", (unsigned long long)cmd_af_xdp.seed_base,
            cmd_af_xdp.seed_set ? "--seed" : (cmd_af_xdp.very_random ? "getrandom" : "CLOCK_BOOTTIME"),
            (unsigned long long)cmd_af_xdp.seed_base);
    for (int i = 0; i < seq_cnt && cmd_af_xdp.literal_payload; ++i)
    {
        int random = 0;
        for (int j = 0; j < cfg->seq[i].pl_cnt; ++j)
            random |= cfg->seq[i].pls[j].exact == NULL && !cfg->seq[i].pls[j].is_static && cfg->seq[i].pls[j].max_len > 0;
        if (cfg->seq[i].pl_cnt > 1 && random)
            fprintf(stderr,
                    "[%d] WARNING - --literal with several payloads follows the declared rule: the shadowed loop "
                    "(sequence.c:552) reads the other payloads' setup lengths, where the reference reads the previous "
                    "iteration's (quirk B8).\n",
                    i + 1);
    }
    if (pcapdump_path) /* no TX path at all: build, pack, write (pcap_dump.h) */
    {
        if (pb_pcap_dump_check(cfg, seq_cnt, &cmd_af_xdp) != 0)
            return EXIT_FAILURE;
        signal(SIGINT, sign_hdl);
        signal(SIGTERM, sign_hdl);
        const int derr = pb_pcap_dump(cfg, seq_cnt, &cmd_af_xdp, pcapdump_path, pcapt0_set, pcapt0_ns);
        free(cfg);
        free(argv_cli);
        pb_config_free();
        return derr ? EXIT_FAILURE : EXIT_SUCCESS;
    }
    pb_pcap_t *pcap = NULL;
    if (cmd_af_xdp.pcap)
    {
        pcap = pb_pcap_open(cmd_af_xdp.pcap);
        if (pcap == NULL)
        {
            fprintf(stderr, "Cannot open pcap file %s.\n", cmd_af_xdp.pcap);
            return EXIT_FAILURE;
        }
        pb_set_tx_hook(pb_pcap_tx, pcap);
    }
    signal(SIGINT, sign_hdl);
    signal(SIGTERM, sign_hdl);
    for (int i = 0; i < seq_cnt && !pb_stop_requested(); ++i)
    {
        seq_send(cfg->interface, cfg->seq[i], (uint16_t)seq_cnt, cmd_af_xdp);
        /* main.c:113 (a second between sequences; PB_SEQ_GAP_MS shortens it for tests) */
        const char *gap = getenv("PB_SEQ_GAP_MS");
        const long ms = gap ? atol(gap) : 1000;
        for (long t = 0; t < ms && !pb_stop_requested(); t += 10)
        {
            struct timespec ts = {0, (ms - t < 10 ? ms - t : 10) * 1000000L};
            nanosleep(&ts, NULL);
        }
    }
    /* shutdown_prog (sequence.c:779-824) without its exit(): the pcap file is closed
     * and the memory freed before returning */
    const int err = pb_shutdown_stats(cfg);
    pb_pcap_close(pcap);
    free(cfg);
    free(argv_cli);
    pb_config_free();
    return err ? EXIT_FAILURE : EXIT_SUCCESS;
}
